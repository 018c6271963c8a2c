// xk_tracker_api.hip.h -- host side of the tracker's front end (xk_trk_*): the fundamental-matrix RANSAC filter of the matches
// (tracker.cpp:233-293, camera.cpp:62-87; xk_fundamental.hip.h) and the pyramidal Lucas-Kanade tracking in front of it
// (tracker.cpp:623-690; xk_klt.hip.h), the FAST detection that produces the features (tracker.cpp:390-590; xk_fast.hip.h) and their
// rotated-BRIEF descriptors (place_recognition.cpp:72-94; xk_orb.hip.h), and the photometric calibration of the images in front of
// all of them (tracker.cpp:761-877, irPhotoCalib.cpp; xk_photo.hip.h).  Behind them, the normalisation and baseline check of the
// track manager's candidate tracks (track_manager.cpp:576-636, camera.cpp; xk_tracks.hip.h).  At the end, Tracker::track itself in
// one call on a resident feature list (tracker.cpp:134-306; xk_frame.hip.h): xk_trk_frame, and xk_trk_photo_frame with calibrateImage,
// which are one body (frame_run).  Last, the whole of TrackManager::manageTracks on tracks that stay on the device
// (track_manager.cpp:115-436; xk_track_store.hip.h): xk_trk_tracks_*, fed from the host or from the block the last frame left.  A stage's launches are queued in one place, by the function its stage entry and the frame both call
// (klt_queue_track, det_queue, orb_queue, trk_queue_ransac, photo_queue_calibrate): it takes what differs as parameters.
// Every stage keeps its buffers in one xk_block (a device block and its pinned mirror, carved once by the stage's setup, which stores
// every pointer an entry needs) and reaches them through the same helpers: sub_of (the stage's setup or XK_EINVAL), img_slot (the
// slot of the previous or the current image or XK_EINVAL), launched (the check behind a group of launches), kept_count_out, setup_install.
// Part of xk_api.hip's translation unit, included at its end.
#pragma once
#include <sched.h>
#include <time.h>

#include "xk_fast.hip.h"
#include "xk_frame.hip.h"
#include "xk_fundamental.hip.h"
#include "xk_klt.hip.h"
#include "xk_orb.hip.h"
#include "xk_photo.hip.h"
#include "xk_photo_spatial.hip.h"
#include "xk_track_store.hip.h"
#include "xk_tracks.hip.h"

#define XKCHK(call)                          \
  do {                                       \
    const int rc_ = (call);                  \
    if (rc_ != XK_OK) return rc_;            \
  } while (0)

static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// "<who>: <what>" as the handle's message
static int fail_at(xk_handle *h, int code, const char *who, const char *what) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return fail(h, code, msg);
}

// the check behind a group of launches
static int launched(xk_handle *h, const char *what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? XK_OK : fail(h, XK_EDEVICE, what, e);
}

// A device block and its pinned mirror: what every stage below allocates once per setup and carves into its buffers.
struct xk_block {
  unsigned char *d, *h;
  size_t d_bytes, h_bytes;
};

static void blk_free(xk_block &b) {
  hipFree(b.d);
  if (b.h) hipHostFree(b.h);
  b = xk_block{};
}

// Both blocks of `who`, zeroed: the pinned one here, the device one on the handle's stream (queued, not waited for).
// The images in these blocks have their rows padded to a pitch.  NO kernel may read the padding columns [w, pitch): xk_klt_pyrdown
// takes four bytes at once only where x + 3 < w, xk_klt_track's plain taps only where the whole window lies inside the image,
// everything else goes through the mirror or a bounds test.  Nothing writes them either (level 0's come from the staging, which copies
// w bytes per row; the blur and the correction write w columns), so they are zeroed once here: a later vectorised load that strays
// into the padding reads zeros, not what was there before.  The same holds for the padding between the pieces of a block.
static int blk_alloc(xk_handle *h, xk_block &b, size_t d_bytes, size_t h_bytes, const char *who) {
  b = xk_block{nullptr, nullptr, d_bytes, h_bytes};
  if (hipMalloc((void **)&b.d, d_bytes) == hipSuccess && hipHostMalloc((void **)&b.h, h_bytes) == hipSuccess &&
      hipMemsetAsync(b.d, 0, d_bytes, h->stream) == hipSuccess) {
    memset(b.h, 0, h_bytes);
    return XK_OK;
  }
  blk_free(b);
  return fail_at(h, XK_ENOMEM, who, "allocation failed");
}

// The next piece of a block: `bytes` at base + off, and off moves on by them rounded up to 16.
template <class T>
static T *carve(unsigned char *base, size_t &off, size_t bytes) {
  T *p = (T *)(base + off);
  off += up16(bytes);
  return p;
}

// The detection setup of an image size (xk_trk_detect_setup): it belongs to the xk_klt whose level-0 images it scans.
struct xk_det {
  int threshold, nms, b, margin, max_candidates;
  int key_cap, wpr;
  size_t lds_bytes;           // of xk_fast_select: the keys, and the blocked mask behind them when both fit
  xk_block blk;                 // device: S | keys | counter | old features | result block | blocked mask (when it does not fit the LDS)
  unsigned char *S;           // pinned: old features in (2 max_matches doubles), then the result block out, at h_res
  unsigned int *keys, *mask_g;
  int *count, *res, *h_res;
  double *old_xy;
  int n_cand;                 // candidates of the last detection (-1: none yet)
};

// The description setup of an image size (xk_trk_describe_setup): it belongs to the xk_klt whose level-0 images it describes.
struct xk_orb {
  int centroid, A, B, edge, max_desc;
  xk_block blk;                 // device: G of slot 0 | G of slot 1 | pattern | keypoints in | kept keypoints | result block
  unsigned char *G[2];        // by slot, as xk_klt::slot: a push swaps the roles of the slots, not their buffers
  int blurred[2];             // G[s] holds the blur of the image in slot s.  xk_trk_push_image clears the flag of the slot it fills
  signed char *pattern;
  int *xy, *kept_xy, *res;
  unsigned char *h_res;       // pinned: keypoints in (2 max_desc ints), then the result block out, at h_res
  signed char h_pattern[1024];
};

// The photometric setup of an image size (xk_trk_photo_setup): it belongs to the xk_klt whose images it calibrates.
struct xk_photo {
  int kernel_size, max_hyp;
  double eps_gap, eps_base;
  xk_block blk;                 // device: raw slot 0 | raw slot 1 | PS | the i/o block | one XkRansacScratch per group
  XkKltPyr raw[2];            // by slot, as xk_klt::slot: the images as pushed.  xk_klt::slot holds the working (corrected) ones
  float *PS;                  // [height][pitch of level 0]
  unsigned char *d_io;        // out: state | value | sum | count | the tracking's result block; in: previous intensities |
                              //   previous points | pixels | o_hist | o_cur | off | frame_back.  blk.h is its mirror, the same layout
  XkPhotoState *st;
  double *value, *prev_int, *o_hist, *o_cur;
  int *sum, *count, *ixy, *off, *frame_back;
  float *pts;
  unsigned char *klt_res;
  XkRansacScratch sc[XK_PHOTO_MAX_GROUPS];
  int ring_n, done;           // host mirrors of the state
  int n_hyp[XK_PHOTO_MAX_GROUPS];   // hypotheses per group of the last call (0: none, or a group of <= 4)
  struct xk_psp *sp;          // xk_trk_photo_spatial_setup; NULL before.  It goes with this setup
};

// The spatial-map setup (xk_trk_photo_spatial_setup): it belongs to the xk_photo whose PS plane it estimates.
struct xk_psp {
  XkPspGrid g;
  int max_count, max_rows, n_max, ld;
  float thr, gp_l, gp_sf, gp_sn;
  xk_block blk;                 // device: counts | coverage | rows | numbering | L | K (and the int32 multiplicities before it) | vectors |
                                //   coarse | the estimated map | state | the staging of one xk_trk_photo_spatial_add.  Pinned: state | staging
  int *count, *sid_hist, *sid_cur, *var_of_cell, *cell_of_var, *deg;
  unsigned char *coverage, *d_in;
  double *b, *L, *K, *c, *x, *alpha, *r, *p, *q, *partial, *diag_l, *diag_k;
  float *coarse, *ps;         // ps: [height][pitch of level 0], as xk_photo::PS
  XkPspState *st;
  size_t in_bytes, cov_bytes;
  hipEvent_t batch;           // behind every batch of launches the host waits for, with a bound
  int state;                  // XK_PSP_ACCUMULATING, _ESTIMATED, _FAILED
  int staged_n;               // n of the last estimate whose intermediates xk_trk_photo_spatial_stage hands out (-1: none)
};

struct xk_klt {
  int width, height, win_w, win_h, max_level, max_iter, levels;    // the first parameter set (win_size_, max_level_, min_eig_thr_)
  double eps, min_eig_thr;
  int has_second, sel;        // xk_trk_klt_second declared a second set; the set xk_trk_track and xk_trk_frame use (xk_trk_klt_select)
  int win_w2, win_h2, max_level2, levels2;                         // the second set (win_size_photo_, ...); max_iter and eps are shared
  double min_eig_thr2;
  int deep;                   // max(levels, levels2): what the slots are laid out for and a push builds
  xk_block blk;                 // device: slot 0 | slot 1 | previous points (floats) | result block
  XkKltPyr slot[2];           // per slot and level: image, dIx, dIy at the level's pitch
  int cur, pushed;            // the slot of the current image; images pushed since the setup, counted to 2
  float *d_pts;
  unsigned char *d_res;       // cur_xy | min_eig | XkKeptPairs | status, packed per call
  unsigned char *h_res;       // pinned: previous points in, then the result block out, at h_res
  unsigned char *h_img;       // pinned: one image at level 0's pitch
  hipEvent_t img_copied;      // the upload out of h_img: the next push waits for it before it refills the staging
  struct xk_det *det;         // xk_trk_detect_setup; NULL before.  It goes with this setup
  struct xk_orb *orb;         // xk_trk_describe_setup; likewise
  struct xk_photo *photo;     // xk_trk_photo_setup; likewise
  struct xk_frm *frm;         // xk_trk_frame_setup; likewise
  size_t slot_bytes;          // of one slot: its levels are one contiguous block
};

// The frame setup (xk_trk_frame_setup): Tracker::track's parameters and the feature list that stays on the device between frames.
// It belongs to the xk_klt whose images it tracks on, and uses the detection and description setups that existed when it was made.
struct xk_frm {
  int n_feat_min, tiles_h, tiles_w, max_per_tile, n_hyp;
  double threshold_px;
  const struct xk_det *det;   // the setups it was made over: a frame asks that they are still the ones in place
  const struct xk_orb *orb;   // NULL: no description
  int n_res;                  // the resident count: the previous frame's matches; -1: the next frame is a first frame
  int cap_det, cap_new;       // the detection's packing bound; the bound of a re-detection's lists (max_desc with a description)
  xk_block blk;                 // device: counts | resident list | pair lists | the stages' result blocks | the frame's result block.  Pinned: the latter
  XkFrameArgs a;              // every device pointer, placed once
  unsigned char *klt_res[2];  // result blocks of the two trackings (klt_res_bytes(max_matches) each)
  unsigned char *fund_res;    // of the outlier removal (trk_res_bytes(max_matches))
  int *orb_res;               // of the description (xk_orb_res_bytes(cap_new)); NULL without one
  struct xk_pfrm *pf;         // xk_trk_photo_frame_setup; NULL before.  It goes with this setup, and with the photo setup it was made over
  int last_m, last_B;         // the matches the last frame left in its result block on the device and the bound that block is laid out by;
  const unsigned char *last_out;   //   last_m -1: no such block (before a frame, after a reset or an error), 0: a first frame's empty list
};

// The photometric frame setup (xk_trk_photo_frame_setup): what Tracker::track of a PHOTOMETRIC_CALI build needs beyond xk_frm.
struct xk_pfrm {
  int n_hyp, threshold;       // the cap of the gain RANSAC; fast_detection_delta_photo_, < 0: no switch
  const struct xk_photo *photo;   // the setup it was made over
  xk_block blk;                 // device: resident and pair intensities | the three intensity lists | truncated pixels | sums, counts |
                                //   the frame's result block.  Pinned: the latter
  double *res_int, *l_iprev, *l_icur, *val1, *val_new, *val2;
  int *ixy1, *ixy2, *sum, *count;
  unsigned char *out;
};

// The baseline setup (xk_trk_baseline_setup): capacities of one batch of tracks.  It belongs to the xk_trk, not to an image size.
struct xk_bl {
  int max_tracks, max_obs;
  xk_block blk;                 // device and pinned, the SAME layout: in: attitudes | trk_off | norm_off | drop_last | observations;
                                //   out: delta_xy | flag | norm_xy.  The variable-length pieces come last in each half
  size_t o_quat, o_trk_off, o_norm_off, o_drop, o_obs, o_delta, o_flag, o_norm;
};

// The track store (xk_trk_tracks_setup): TrackManager's lists on the device.  It belongs to the xk_trk, as the baseline setup.
struct xk_ts {
  int max_tracks, max_n;      // max_n: the xk_trk's max_matches, the most matches of a call
  xk_block blk;                 // device: store | scratch | a call's inputs | result block | the lists entry's gather.  Pinned: inputs | result block
  XkTsArgs a;                 // the store's and the scratch's device pointers, placed once
  unsigned char *d_in, *d_out, *d_gather;
  size_t in_bytes, out_bytes, gather_bytes;
  int n_slam, n_new, n_opp;   // host mirrors of the list lengths, from the last result block and the removals since
};

struct xk_trk {
  xk_handle *h;
  int max_matches;
  double fx, fy, cx, cy, s, s_term;
  xk_block blk;                 // device: distorted / undistorted / float-cast points [4 max_matches doubles] each, XkRansacScratch, result block
  double *dist, *und, *pts;
  XkRansacScratch sc;
  unsigned char *d_res;       // the result block: F | XkKeptPairs | mask, packed per call
  unsigned char *h_res;       // pinned: points in (4 max_matches doubles), then the result block out, at h_res
  int n_hyp;                  // hypotheses of the last RANSAC or LMedS stage call (0: none yet)
  int method;                 // XK_TRK_RANSAC or XK_TRK_LMEDS: what xk_trk_filter_matches and the frames run (xk_trk_outlier_method)
  int lmeds_hyp;              // hypotheses of the last call if it was LMedS, stage entry or frame (0: it was not): their medians are in sc.sum
  const double *lmeds_last;   // device: that call's winner's median and sigma
  int model;                  // XK_CAM_FOV, XK_CAM_RADTAN or XK_CAM_EQUIDISTANT: what every undistortion applies (xk_trk_camera_model)
  double cam_k[5];            // that model's coefficients (unused under XK_CAM_FOV: s and s_term above)
  int *cam_cnt;               // device [2]: invalid points and the largest step count of the last undistortion under another model than FOV
  struct xk_klt *klt;         // the feature tracking in front of the filter (xk_trk_klt_setup); NULL before
  struct xk_bl *bl;           // the baseline check of the track manager's candidates (xk_trk_baseline_setup); NULL before
  struct xk_ts *ts;           // the track manager's lists on the device (xk_trk_tracks_setup); NULL before
};

// the result blocks for n pairs: F [9] | kept pairs | mask [n], and cur_xy [n][2] | min_eig [n] | kept pairs | status [n]
static size_t trk_res_bytes(int n) { return sizeof(double) * 9 + xk_kept_pairs_bytes(n) + (size_t)n; }
// LMedS adds its winner's median and sigma behind that block, at the next multiple of 8: nothing in front of them moves
static size_t trk_lmeds_off(int n) { return (trk_res_bytes(n) + 7) & ~(size_t)7; }
static size_t trk_res_total(int n) { return trk_lmeds_off(n) + 2 * sizeof(double); }
static size_t klt_res_bytes(int n) { return sizeof(double) * 3 * (size_t)n + xk_kept_pairs_bytes(n) + (size_t)n; }

// The count at `at` in a result block's pinned copy: 0 <= count <= n, or XK_EDEVICE.
static int kept_count_out(xk_handle *h, const char *who, const void *at, int n, int *n_kept) {
  int kept = 0;
  memcpy(&kept, at, sizeof(int));
  if (kept < 0 || kept > n) return fail_at(h, XK_EDEVICE, who, "kept count out of range");
  *n_kept = kept;
  return XK_OK;
}

// The kept pairs of a result block out of its pinned copy r (the device block starts at d_res).
static int kept_pairs_out(xk_handle *h, const char *who, const XkKeptPairs &k, const unsigned char *d_res, const unsigned char *r, int n,
                          int *keep_idx, double *prev_xy, double *cur_xy, int *n_kept) {
  XKCHK(kept_count_out(h, who, r + ((unsigned char *)k.res - d_res), n, n_kept));
  memcpy(keep_idx, r + ((unsigned char *)k.keep_idx - d_res), sizeof(int) * (size_t)*n_kept);
  memcpy(prev_xy, r + ((unsigned char *)k.kept_prev - d_res), sizeof(double) * 2 * (size_t)*n_kept);
  memcpy(cur_xy, r + ((unsigned char *)k.kept_cur - d_res), sizeof(double) * 2 * (size_t)*n_kept);
  return XK_OK;
}

// xk_det, xk_orb, xk_photo: a block and nothing else to give back
template <class T>
static void setup_free(T *p) {
  if (!p) return;
  blk_free(p->blk);
  free(p);
}

static void setup_free(xk_psp *s) {
  if (!s) return;
  if (s->batch) hipEventDestroy(s->batch);
  blk_free(s->blk);
  free(s);
}

static void setup_free(xk_frm *f) {
  if (!f) return;
  setup_free(f->pf);
  blk_free(f->blk);
  free(f);
}

static void setup_free(xk_photo *p) {
  if (!p) return;
  setup_free(p->sp);
  blk_free(p->blk);
  free(p);
}

static void setup_free(xk_klt *k) {
  if (!k) return;
  setup_free(k->det);
  setup_free(k->orb);
  setup_free(k->photo);
  setup_free(k->frm);
  blk_free(k->blk);
  if (k->h_img) hipHostFree(k->h_img);
  if (k->img_copied) hipEventDestroy(k->img_copied);
  free(k);
}

// The end of every setup.  The new state was built whole (rc says how that went); one wait, after which the staging is free and the
// old state idle; then the old one goes and the new one takes its place.  A failure leaves the old one where it is.
template <class T>
static int setup_install(xk_handle *h, int rc, const char *who, T *&old, T *fresh) {
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == XK_OK) rc = fail_at(h, XK_ENOMEM, who, "allocation failed");
  if (rc != XK_OK) {
    setup_free(fresh);
    return rc;
  }
  setup_free(old);
  old = fresh;
  return XK_OK;
}

// The setup of entry `who` that `setup` makes (xk_klt::det, orb or photo), or nullptr after fail(XK_EINVAL).
template <class T>
static T *sub_of(xk_trk *t, T *xk_klt::*sub, const char *who, const char *setup) {
  T *p = t->klt ? t->klt->*sub : nullptr;
  if (!p) {
    char what[64];
    snprintf(what, sizeof what, "before %s", setup);
    fail_at(t->h, XK_EINVAL, who, what);
  }
  return p;
}

// The slot of the previous (which = 0) or the current (1) image for entry `who`, or -1 after fail(XK_EINVAL).
static int img_slot(xk_trk *t, const char *who, int which) {
  const xk_klt *k = t->klt;
  const char *what = !k ? "before xk_trk_klt_setup" : which < 0 || which > 1 ? "which is 0 or 1" :
                     k->pushed < 2 - which ? "that image has not been pushed" : nullptr;
  if (!what) return which == 1 ? k->cur : k->cur ^ 1;
  fail_at(t->h, XK_EINVAL, who, what);
  return -1;
}

// A frame setup was made over the detection and description setups in place: when one of them is replaced it goes (the stream is idle:
// setup_install has waited).
static void frame_drop(xk_klt *k) {
  setup_free(k->frm);
  k->frm = nullptr;
}

// The slot's plane that a push fills first: the raw one with a photo setup, the only one without.
static const XkKltPyr &photo_raw_slot(const xk_klt *k, int s) { return k->photo ? k->photo->raw[s] : k->slot[s]; }

// ---------------------------------------------------------------------------
// Fundamental-matrix RANSAC filter of the tracker's matches (tracker.cpp:233-293, camera.cpp:62-87), xk_fundamental.hip.h
// ---------------------------------------------------------------------------
extern "C" void xk_trk_destroy(xk_trk *t) {
  if (!t) return;
  if (t->klt || t->bl || t->ts) hipStreamSynchronize(t->h->stream);
  setup_free(t->klt);
  setup_free(t->bl);
  setup_free(t->ts);
  blk_free(t->blk);
  free(t);
}

extern "C" int xk_trk_create(xk_handle *h, int max_matches, double fx, double fy, double cx, double cy, double s, xk_trk **out) {
  if (!h || !out) return XK_EINVAL;
  if (max_matches < 1) return fail(h, XK_EINVAL, "xk_trk_create: max_matches < 1");
  if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(s))
    return fail(h, XK_EINVAL, "xk_trk_create: focal lengths must be positive and the intrinsics finite");
  HIPCHK(h, hipSetDevice(h->device));
  xk_trk *t = (xk_trk *)calloc(1, sizeof(xk_trk));
  if (!t) return XK_ENOMEM;
  t->h = h; t->max_matches = max_matches;
  t->fx = fx; t->fy = fy; t->cx = cx; t->cy = cy; t->s = s;
  t->s_term = s != 0.0 ? 1.0 / (2.0 * std::tan(s / 2.0)) : 0.0;        // camera.cpp:39
  const size_t pts = sizeof(double) * 4 * (size_t)max_matches;
  const size_t head = 3 * pts + xk_ransac_scratch_bytes<XK_FUND_MAXC>(XK_FUND_MAX_HYP);
  const size_t cnt_off = (head + trk_res_total(max_matches) + 7) & ~(size_t)7;          // the two counters, behind everything else
  const int rc = blk_alloc(h, t->blk, cnt_off + 2 * sizeof(int), pts + trk_res_total(max_matches), "xk_trk_create");
  if (rc != XK_OK) {
    free(t);
    return rc;
  }
  size_t off = 0;
  t->dist = carve<double>(t->blk.d, off, pts); t->und = carve<double>(t->blk.d, off, pts); t->pts = carve<double>(t->blk.d, off, pts);
  t->sc = xk_ransac_scratch<XK_FUND_MAXC>(t->blk.d + off, XK_FUND_MAX_HYP);
  t->d_res = t->blk.d + head;                                            // (a multiple of 8: doubles first, and the scratch is not padded)
  t->h_res = t->blk.h + pts;
  t->cam_cnt = (int *)(t->blk.d + cnt_off);
  t->method = XK_TRK_RANSAC;
  t->model = XK_CAM_FOV;
  *out = t;
  return XK_OK;
}

static_assert(XK_CAM_FOV == XK_CAM_MODEL_FOV && XK_CAM_RADTAN == XK_CAM_MODEL_RADTAN && XK_CAM_EQUIDISTANT == XK_CAM_MODEL_EQUIDISTANT,
              "include/xk.h and xk_camera.h number the camera models alike");

// The outlier removal of n pairs whose result block (trk_res_total(n)) starts at d_res: the stage entries' t->d_res or a frame's.  With
// n_dev the count is the device's and n the bound the block is laid out by.  The camera model goes with it: this is the one place every
// undistortion, stage entry or frame, takes it from.
static XkFundArgs trk_args(xk_trk *t, unsigned char *d_res, int n, const int *n_dev = nullptr) {
  XkFundArgs a{};
  a.dist = t->dist; a.und = t->und; a.pts = t->pts; a.sc = t->sc;
  a.F = (double *)d_res;
  a.kept = xk_kept_pairs(a.F + 9, n);
  a.mask = xk_kept_pairs_end(a.kept, n);
  a.lmeds = (double *)(d_res + trk_lmeds_off(n));
  a.n = n; a.n_pts = 2 * n; a.n_dev = n_dev;
  a.fx = t->fx; a.fy = t->fy; a.cx = t->cx; a.cy = t->cy; a.s = t->s; a.s_term = t->s_term;
  a.model = t->model;
  if (t->model != XK_CAM_FOV) {
    memcpy(a.cam_k, t->cam_k, sizeof a.cam_k);
    a.cam_cnt = t->cam_cnt;
  }
  return a;
}

// Camera::undistort of a.n_pts points, queued.  Under another model than FOV the two counters are cleared in front of the kernel.
static void trk_queue_undistort(xk_handle *h, const XkFundArgs &a) {
  if (a.cam_cnt) hipMemsetAsync(a.cam_cnt, 0, 2 * sizeof(int), h->stream);
  hipLaunchKernelGGL(xk_fund_undistort, dim3((a.n_pts + 255) / 256), dim3(256), 0, h->stream, a);
}

// The outlier removal of a's pairs by `method`, queued: Camera::undistort of both lists first (undistort = true), then solve, score and
// mask (RANSAC) or solve, median and mask (LMedS, which ignores threshold_px).  Three launches either way, four with the undistortion.
static int trk_queue_ransac(xk_handle *h, XkFundArgs &a, int method, bool undistort, double threshold_px, int n_hyp, unsigned long seed) {
  const bool lmeds = method == XK_TRK_LMEDS;
  a.n_hyp = n_hyp;
  a.t2 = threshold_px * threshold_px;
  a.seed = (unsigned long long)seed;
  a.min_n = lmeds ? 8 : 7;
  if (undistort) trk_queue_undistort(h, a);
  hipLaunchKernelGGL(xk_fund_solve, dim3((n_hyp + XK_FUND_SOLVE_T - 1) / XK_FUND_SOLVE_T), dim3(XK_FUND_SOLVE_T), 0, h->stream, a);
  if (lmeds) {
    hipLaunchKernelGGL(xk_fund_median, dim3(n_hyp), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(xk_fund_mask_lmeds, dim3(1), dim3(256), 0, h->stream, a);
  } else {
    hipLaunchKernelGGL(xk_fund_score, dim3(n_hyp), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(xk_fund_mask, dim3(1), dim3(256), 0, h->stream, a);
  }
  return launched(h, lmeds ? "fundamental LMedS launch" : "fundamental RANSAC launch");
}

// What xk_trk_fundamental_medians reads after the call that `method` ran with n_hyp hypotheses on the result block at d_res for n pairs
// (n_hyp = 0: nothing ran).
static void trk_note_call(xk_trk *t, int method, int n_hyp, const unsigned char *d_res, int n) {
  t->lmeds_hyp = method == XK_TRK_LMEDS ? n_hyp : 0;
  t->lmeds_last = (const double *)(d_res + trk_lmeds_off(n));
}

/* Camera::undistort (camera.cpp:62-87) */
extern "C" int xk_trk_undistort(xk_trk *t, const double *dist_xy, int n, double *xy) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  if (n < 0 || (n > 0 && (!dist_xy || !xy))) return fail(h, XK_EINVAL, "xk_trk_undistort: null argument or negative n");
  if (n > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_undistort: more points than max_matches");
  if (n == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  XkFundArgs a = trk_args(t, t->d_res, 0);
  a.n_pts = n;
  memcpy(t->blk.h, dist_xy, sizeof(double) * 2 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync((void *)a.dist, t->blk.h, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  trk_queue_undistort(h, a);
  XKCHK(launched(h, "undistort launch"));
  HIPCHK(h, hipMemcpyAsync(t->blk.h, a.und, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(xy, t->blk.h, sizeof(double) * 2 * (size_t)n);
  return XK_OK;
}

/* The camera model of every undistortion from the next call on */
extern "C" int xk_trk_camera_model(xk_trk *t, int model, const double *coeffs, int n_coeffs) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  const bool count_ok = model == XK_CAM_FOV ? n_coeffs == 1 : model == XK_CAM_RADTAN ? (n_coeffs == 4 || n_coeffs == 5) :
                        model == XK_CAM_EQUIDISTANT ? n_coeffs == 4 : false;
  if (!coeffs || !count_ok)
    return fail(h, XK_EINVAL, "xk_trk_camera_model: model is 0 (FOV, 1 coefficient), 1 (radial-tangential, 4 or 5) or 2 (equidistant, 4)");
  for (int i = 0; i < n_coeffs; ++i)
    if (!std::isfinite(coeffs[i])) return fail(h, XK_EINVAL, "xk_trk_camera_model: coefficient not finite");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(t->cam_cnt, 0, 2 * sizeof(int), h->stream));   // (what xk_trk_undistort_status reports until the next undistortion)
  t->model = model;
  memset(t->cam_k, 0, sizeof t->cam_k);
  if (model == XK_CAM_FOV) {
    t->s = coeffs[0];
    t->s_term = t->s != 0.0 ? 1.0 / (2.0 * std::tan(t->s / 2.0)) : 0.0;  // camera.cpp:39, as xk_trk_create
  } else {
    memcpy(t->cam_k, coeffs, sizeof(double) * (size_t)n_coeffs);
  }
  return XK_OK;
}

/* The forward map of the camera model: undistorted pixels -> distorted pixels */
extern "C" int xk_trk_distort(xk_trk *t, const double *xy, int n, double *dist_xy) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  if (n < 0 || (n > 0 && (!xy || !dist_xy))) return fail(h, XK_EINVAL, "xk_trk_distort: null argument or negative n");
  if (n > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_distort: more points than max_matches");
  if (n == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  XkFundArgs a = trk_args(t, t->d_res, 0);
  a.n_pts = n;
  memcpy(t->blk.h, xy, sizeof(double) * 2 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync((void *)a.und, t->blk.h, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_cam_distort, dim3((n + 255) / 256), dim3(256), 0, h->stream, a);
  XKCHK(launched(h, "distort launch"));
  HIPCHK(h, hipMemcpyAsync(t->blk.h, a.pts, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(dist_xy, t->blk.h, sizeof(double) * 2 * (size_t)n);
  return XK_OK;
}

/* The counters of the last undistortion: an inspection path with a copy and a wait of its own */
extern "C" int xk_trk_undistort_status(xk_trk *t, int *n_invalid, int *max_steps) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  int cnt[2] = {0, 0};
  if (t->model != XK_CAM_FOV && (n_invalid || max_steps)) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(cnt, t->cam_cnt, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (n_invalid) *n_invalid = cnt[0];
  if (max_steps) *max_steps = cnt[1];
  return XK_OK;
}

// The launches behind both RANSAC entries: the points are in the pinned block (4n doubles: previous, then current), distorted
// (undistort = true: they go through xk_fund_undistort) or already what the RANSAC sees.  One copy in, one copy out, one wait.
static int trk_run(xk_trk *t, XkFundArgs &a, int method, bool undistort, double threshold_px, int n_hyp, unsigned long seed) {
  xk_handle *h = t->h;
  const int n = a.n;
  if (!undistort) a.und = a.pts;
  t->n_hyp = 0;
  trk_note_call(t, method, 0, t->d_res, n);
  HIPCHK(h, hipMemcpyAsync((void *)(undistort ? a.dist : a.pts), t->blk.h, sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  XKCHK(trk_queue_ransac(h, a, method, undistort, threshold_px, n_hyp, seed));
  HIPCHK(h, hipMemcpyAsync(t->h_res, t->d_res, method == XK_TRK_LMEDS ? trk_res_total(n) : trk_res_bytes(n), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  t->n_hyp = n_hyp;
  trk_note_call(t, method, n_hyp, t->d_res, n);
  return XK_OK;
}

static int trk_check(xk_trk *t, const char *who, int n, double threshold_px, int n_hyp, bool nulls) {
  const char *what = nullptr;
  int rc = XK_EINVAL;
  if (nulls || n < 0) what = "null argument or negative n";
  else if (!(threshold_px >= 0.0) || !std::isfinite(threshold_px)) what = "threshold_px < 0";
  else if (n_hyp < 1 || n_hyp > XK_FUND_MAX_HYP) what = "n_hyp outside 1...4096";
  else if (n > t->max_matches) { what = "more point pairs than max_matches"; rc = XK_ECAPACITY; }
  return what ? fail_at(t->h, rc, who, what) : XK_OK;
}

/* cv::findFundamentalMat(pts1, pts2, cv::RANSAC, 0.3, 0.99, mask) (tracker.cpp:243-260) */
extern "C" int xk_trk_fundamental_ransac(xk_trk *t, const float *prev_xy, const float *cur_xy, int n, double threshold_px, int n_hyp,
                                         unsigned long seed, unsigned char *mask, double *F, int *n_inliers) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  XKCHK(trk_check(t, "xk_trk_fundamental_ransac", n, threshold_px, n_hyp, !mask || !n_inliers || (n > 0 && (!prev_xy || !cur_xy))));
  *n_inliers = 0;
  memset(mask, 0, (size_t)n);
  if (F) memset(F, 0, 9 * sizeof(double));
  if (n < 7) { t->n_hyp = t->lmeds_hyp = 0; return XK_OK; }  // (OpenCV returns an empty mask: the loop of :263-268 keeps nothing; no hypotheses)
  HIPCHK(h, hipSetDevice(h->device));
  XkFundArgs a = trk_args(t, t->d_res, n);
  double *h_pts = (double *)t->blk.h;
  for (size_t i = 0; i < 2 * (size_t)n; ++i) { h_pts[i] = (double)prev_xy[i]; h_pts[2 * (size_t)n + i] = (double)cur_xy[i]; }
  XKCHK(trk_run(t, a, XK_TRK_RANSAC, false, threshold_px, n_hyp, seed));
  const unsigned char *r = t->h_res;
  if (F) memcpy(F, r, 9 * sizeof(double));
  memcpy(n_inliers, r + ((unsigned char *)a.kept.res - t->d_res), sizeof(int));
  memcpy(mask, r + (a.mask - t->d_res), (size_t)n);
  return XK_OK;
}

/* cv::findFundamentalMat(pts1, pts2, cv::LMEDS, ., 0.99, mask): the outlier_method a configuration may name (tracker.h:256) */
extern "C" int xk_trk_outlier_method(xk_trk *t, int method) {
  if (!t) return XK_EINVAL;
  if (method != XK_TRK_RANSAC && method != XK_TRK_LMEDS) return fail(t->h, XK_EINVAL, "xk_trk_outlier_method: method is 8 (RANSAC) or 4 (LMedS)");
  t->method = method;
  return XK_OK;
}

extern "C" int xk_trk_fundamental_lmeds(xk_trk *t, const float *prev_xy, const float *cur_xy, int n, int n_hyp, unsigned long seed,
                                        unsigned char *mask, double *F, int *n_inliers, double *median, double *sigma) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  XKCHK(trk_check(t, "xk_trk_fundamental_lmeds", n, 0.0, n_hyp, !mask || !n_inliers || (n > 0 && (!prev_xy || !cur_xy))));
  *n_inliers = 0;
  memset(mask, 0, (size_t)n);
  if (F) memset(F, 0, 9 * sizeof(double));
  if (median) *median = 0.0;
  if (sigma) *sigma = 0.0;
  if (n < 8) { t->n_hyp = t->lmeds_hyp = 0; return XK_OK; }  // (the scale needs n - 7 > 0)
  HIPCHK(h, hipSetDevice(h->device));
  XkFundArgs a = trk_args(t, t->d_res, n);
  double *h_pts = (double *)t->blk.h;
  for (size_t i = 0; i < 2 * (size_t)n; ++i) { h_pts[i] = (double)prev_xy[i]; h_pts[2 * (size_t)n + i] = (double)cur_xy[i]; }
  XKCHK(trk_run(t, a, XK_TRK_LMEDS, false, 0.0, n_hyp, seed));
  const unsigned char *r = t->h_res;
  if (F) memcpy(F, r, 9 * sizeof(double));
  memcpy(n_inliers, r + ((unsigned char *)a.kept.res - t->d_res), sizeof(int));
  memcpy(mask, r + (a.mask - t->d_res), (size_t)n);
  if (median) memcpy(median, r + trk_lmeds_off(n), sizeof(double));
  if (sigma) memcpy(sigma, r + trk_lmeds_off(n) + sizeof(double), sizeof(double));
  return XK_OK;
}

/* The medians of hypotheses first ... first+count-1 of the last call if it was LMedS (+inf: not a candidate), and its winner's median and sigma */
extern "C" int xk_trk_fundamental_medians(xk_trk *t, int first, int count, double *median, double *last) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  if (first < 0 || count < 0) return fail(h, XK_EINVAL, "xk_trk_fundamental_medians: negative range");
  if (t->lmeds_hyp < 1 || first + (long)count > t->lmeds_hyp)
    return fail(h, XK_EINVAL, "xk_trk_fundamental_medians: range outside the hypotheses of the last call, or that call was not LMedS");
  if ((count == 0 || !median) && !last) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (median && count > 0)
    HIPCHK(h, hipMemcpyAsync(median, t->sc.sum + (size_t)first * XK_FUND_MAXC, sizeof(double) * XK_FUND_MAXC * (size_t)count, hipMemcpyDeviceToHost,
                             h->stream));
  if (last) HIPCHK(h, hipMemcpyAsync(last, t->lmeds_last, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// One model per hypothesis slot, as its only candidate: what xk_fund_score and xk_fund_median then score.  (The models are in place:
// the copy put model j at cand[j][0].)
__global__ __launch_bounds__(256) void xk_fund_models(XkFundArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) *a.sc.key = 0ull;
  if (j >= a.n_hyp) return;
  double *F = a.sc.cand + (size_t)j * (XK_FUND_MAXC * 9);
  for (int i = 9; i < XK_FUND_MAXC * 9; ++i) F[i] = 0.0;
  a.sc.ncand[j] = 1;
}

/* The m models F, as given, under both criteria: the inlier count at threshold_px and the median of the errors of the n pairs */
extern "C" int xk_trk_fundamental_score(xk_trk *t, const float *prev_xy, const float *cur_xy, int n, const double *F, int m, double threshold_px,
                                        int *inliers, double *median) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  XKCHK(trk_check(t, "xk_trk_fundamental_score", n, threshold_px, m, !prev_xy || !cur_xy || !F || !inliers || !median));
  if (n < 1) return fail(h, XK_EINVAL, "xk_trk_fundamental_score: n < 1");
  HIPCHK(h, hipSetDevice(h->device));
  XkFundArgs a = trk_args(t, t->d_res, n);
  a.n_hyp = m; a.t2 = threshold_px * threshold_px; a.min_n = 1;
  t->n_hyp = t->lmeds_hyp = 0;                                // (the scratch no longer holds a filter's hypotheses)
  double *h_pts = (double *)t->blk.h;
  for (size_t i = 0; i < 2 * (size_t)n; ++i) { h_pts[i] = (double)prev_xy[i]; h_pts[2 * (size_t)n + i] = (double)cur_xy[i]; }
  const size_t slot = sizeof(double) * XK_FUND_MAXC * 9, row = sizeof(double) * XK_FUND_MAXC, irow = sizeof(int) * XK_FUND_MAXC;
  HIPCHK(h, hipMemcpyAsync((void *)a.pts, t->blk.h, sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(a.sc.cand, slot, F, sizeof(double) * 9, sizeof(double) * 9, (size_t)m, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_fund_models, dim3((m + 255) / 256), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(xk_fund_score, dim3(m), dim3(256), 0, h->stream, a);
  XKCHK(launched(h, "fundamental score launch"));
  HIPCHK(h, hipMemcpy2DAsync(inliers, sizeof(int), a.sc.cnt, irow, sizeof(int), (size_t)m, hipMemcpyDeviceToHost, h->stream));
  hipLaunchKernelGGL(xk_fund_median, dim3(m), dim3(256), 0, h->stream, a);      // (it zeroes sc.cnt: the counts are on their way out)
  XKCHK(launched(h, "fundamental median launch"));
  HIPCHK(h, hipMemcpy2DAsync(median, sizeof(double), a.sc.sum, row, sizeof(double), (size_t)m, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

/* What the last RANSAC of the tracker's matches (tracker.cpp:259-260) left for hypotheses first ... first+count-1 */
extern "C" int xk_trk_fundamental_hypotheses(xk_trk *t, int first, int count, int *n_cand, double *F, int *inliers) {
  if (!t) return XK_EINVAL;
  return ransac_hypotheses(t->h, "xk_trk_fundamental_hypotheses", "RANSAC", t->n_hyp, t->sc, XK_FUND_MAXC, first, count,
                           n_cand, F, inliers);
}

/* The outlier removal of Tracker::track (tracker.cpp:233-293): undistort both lists, RANSAC, keep the masked pairs */
extern "C" int xk_trk_filter_matches(xk_trk *t, const double *prev_dist_xy, const double *cur_dist_xy, int n, double threshold_px,
                                     int n_hyp, unsigned long seed, unsigned char *mask, int *keep_idx, double *prev_xy, double *cur_xy,
                                     int *n_inliers) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  XKCHK(trk_check(t, "xk_trk_filter_matches", n, threshold_px, n_hyp,
                     !mask || !keep_idx || !prev_xy || !cur_xy || !n_inliers || (n > 0 && (!prev_dist_xy || !cur_dist_xy))));
  *n_inliers = 0;
  memset(mask, 0, (size_t)n);
  if (n < (t->method == XK_TRK_LMEDS ? 8 : 7)) { t->n_hyp = t->lmeds_hyp = 0; return XK_OK; }
  HIPCHK(h, hipSetDevice(h->device));
  XkFundArgs a = trk_args(t, t->d_res, n);
  memcpy(t->blk.h, prev_dist_xy, sizeof(double) * 2 * (size_t)n);
  memcpy(t->blk.h + sizeof(double) * 2 * (size_t)n, cur_dist_xy, sizeof(double) * 2 * (size_t)n);
  XKCHK(trk_run(t, a, t->method, true, threshold_px, n_hyp, seed));
  const unsigned char *r = t->h_res;
  XKCHK(kept_pairs_out(h, "xk_trk_filter_matches", a.kept, t->d_res, r, n, keep_idx, prev_xy, cur_xy, n_inliers));
  memcpy(mask, r + (a.mask - t->d_res), (size_t)n);
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Pyramidal Lucas-Kanade tracking of the tracker's features (tracker.cpp:623-690), xk_klt.hip.h
// ---------------------------------------------------------------------------
// The planes of a slot's levels (w, h and pitch are set) from `base` on: per level the image, then dIx and dIy.
static void klt_place(XkKltPyr &P, int levels, unsigned char *base) {
  for (int l = 0; l <= levels; ++l) {
    XkKltLevel &L = P.lv[l];
    const size_t plane = (size_t)L.pitch * L.h;
    L.img = base; L.dx = (short *)(base + plane); L.dy = (short *)(base + 3 * plane);
    base += 5 * plane;
  }
}

// Rule 1 of DESIGN 3.11: the largest l <= max_level with W_k > win_w and H_k > win_h for every k <= l; -1 if level 0 fails.
static int klt_count_levels(int w, int h, int win_w, int win_h, int max_level) {
  int lv = -1;
  for (int l = 0; l <= max_level && w > win_w && h > win_h; ++l) { lv = l; w = (w + 1) / 2; h = (h + 1) / 2; }
  return lv;
}

// One parameter set's checks for entry `who`: its levels by rule 1, or -1 after fail(XK_EINVAL).
static int klt_set_levels(xk_handle *h, const char *who, int width, int height, int win_w, int win_h, int max_level, double min_eig_thr) {
  const char *what = win_w < 3 || win_w > XK_KLT_MAX_WIN || win_h < 3 || win_h > XK_KLT_MAX_WIN ? "window outside 3...31" :
                     max_level < 0 || max_level >= XK_KLT_MAX_LEVELS ? "max_level outside 0...4" :
                     !(min_eig_thr >= 0.0) || !std::isfinite(min_eig_thr) ? "min_eig_thr < 0" : nullptr;
  const int levels = what ? -1 : klt_count_levels(width, height, win_w, win_h, max_level);
  if (!what && levels < 0) what = "the window does not fit the image";
  if (what) fail_at(h, XK_EINVAL, who, what);
  return levels;
}

// The setup behind xk_trk_klt_setup and xk_trk_klt_second: `par` holds the checked parameters (both sets' levels and `deep` included); the
// buffers of two images are laid out for par.deep levels, and the new setup replaces the old one with everything that hangs on it.
static int klt_make(xk_trk *t, const xk_klt &par, const char *who) {
  xk_handle *h = t->h;
  const int width = par.width, height = par.height, levels = par.deep;
  HIPCHK(h, hipSetDevice(h->device));
  xk_klt *k = (xk_klt *)calloc(1, sizeof(xk_klt));
  if (!k) return XK_ENOMEM;
  k->width = width; k->height = height; k->win_w = par.win_w; k->win_h = par.win_h; k->max_level = par.max_level; k->max_iter = par.max_iter;
  k->levels = par.levels; k->eps = par.eps; k->min_eig_thr = par.min_eig_thr;
  k->has_second = par.has_second; k->sel = 0;
  k->win_w2 = par.win_w2; k->win_h2 = par.win_h2; k->max_level2 = par.max_level2; k->levels2 = par.levels2; k->min_eig_thr2 = par.min_eig_thr2;
  k->deep = levels;
  k->cur = 0; k->pushed = 0;
  XkKltPyr P{};                                                   // per level: pitch h bytes of image, then two planes of shorts
  for (int l = 0, w = width, hh = height; l <= levels; ++l, w = (w + 1) / 2, hh = (hh + 1) / 2) {
    P.lv[l].w = w; P.lv[l].h = hh; P.lv[l].pitch = round_up(w, 16);
    k->slot_bytes += 5 * (size_t)P.lv[l].pitch * hh;
  }
  const size_t pts_bytes = up16(sizeof(float) * 2 * (size_t)t->max_matches), res_bytes = klt_res_bytes(t->max_matches);
  const size_t img_bytes = (size_t)P.lv[0].pitch * height;
  int rc = blk_alloc(h, k->blk, 2 * k->slot_bytes + pts_bytes + res_bytes, pts_bytes + res_bytes, who);
  if (rc == XK_OK && (hipHostMalloc((void **)&k->h_img, img_bytes) != hipSuccess ||
                      hipEventCreateWithFlags(&k->img_copied, hipEventDisableTiming) != hipSuccess))
    rc = fail_at(h, XK_ENOMEM, who, "allocation failed");
  if (rc == XK_OK) {
    memset(k->h_img, 0, img_bytes);                               // (the staging's padding columns, as blk_alloc's)
    size_t off = 0;
    for (int s = 0; s < 2; ++s) {
      k->slot[s] = P;
      klt_place(k->slot[s], levels, carve<unsigned char>(k->blk.d, off, k->slot_bytes));
    }
    k->d_pts = carve<float>(k->blk.d, off, pts_bytes);
    k->d_res = k->blk.d + off;
    k->h_res = k->blk.h + pts_bytes;
  }
  return setup_install(h, rc, who, t->klt, k);                            // (the old setup's detection, description and photo setups go with it)
}

/* The parameters of cv::calcOpticalFlowPyrLK as Tracker holds them (tracker.h:234-261) and the device buffers of two images */
extern "C" int xk_trk_klt_setup(xk_trk *t, int width, int height, int win_w, int win_h, int max_level, int max_iter, double eps,
                                double min_eig_thr) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  if (width < 16 || width > 4096 || height < 16 || height > 4096) return fail(h, XK_EINVAL, "xk_trk_klt_setup: image size outside 16...4096");
  if (win_w < 3 || win_w > XK_KLT_MAX_WIN || win_h < 3 || win_h > XK_KLT_MAX_WIN) return fail(h, XK_EINVAL, "xk_trk_klt_setup: window outside 3...31");
  if (max_level < 0 || max_level >= XK_KLT_MAX_LEVELS) return fail(h, XK_EINVAL, "xk_trk_klt_setup: max_level outside 0...4");
  if (max_iter < 1 || max_iter > 100) return fail(h, XK_EINVAL, "xk_trk_klt_setup: max_iter outside 1...100");
  if (!(eps > 0.0) || !(eps <= 10.0)) return fail(h, XK_EINVAL, "xk_trk_klt_setup: eps outside (0, 10]");
  if (!(min_eig_thr >= 0.0) || !std::isfinite(min_eig_thr)) return fail(h, XK_EINVAL, "xk_trk_klt_setup: min_eig_thr < 0");
  const int levels = klt_count_levels(width, height, win_w, win_h, max_level);
  if (levels < 0) return fail(h, XK_EINVAL, "xk_trk_klt_setup: the window does not fit the image");
  xk_klt par{};
  par.width = width; par.height = height; par.win_w = win_w; par.win_h = win_h; par.max_level = max_level; par.max_iter = max_iter;
  par.levels = par.deep = levels; par.eps = eps; par.min_eig_thr = min_eig_thr;
  return klt_make(t, par, "xk_trk_klt_setup");
}

/* The second parameter set of a PHOTOMETRIC_CALI build (win_size_photo_, max_level_photo_, min_eig_thr_photo_; tracker.cpp:641-651).  A
 * setup-class call: the slots are laid out again for the deeper of the two sets, the images are forgotten and the dependent setups go */
extern "C" int xk_trk_klt_second(xk_trk *t, int win_w, int win_h, int max_level, double min_eig_thr) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  const xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_klt_second: before xk_trk_klt_setup");
  const int levels2 = klt_set_levels(h, "xk_trk_klt_second", k->width, k->height, win_w, win_h, max_level, min_eig_thr);
  if (levels2 < 0) return XK_EINVAL;
  xk_klt par{};
  par.width = k->width; par.height = k->height; par.win_w = k->win_w; par.win_h = k->win_h; par.max_level = k->max_level;
  par.max_iter = k->max_iter; par.levels = k->levels; par.eps = k->eps; par.min_eig_thr = k->min_eig_thr;
  par.has_second = 1; par.win_w2 = win_w; par.win_h2 = win_h; par.max_level2 = max_level; par.levels2 = levels2; par.min_eig_thr2 = min_eig_thr;
  par.deep = std::max(k->levels, levels2);
  return klt_make(t, par, "xk_trk_klt_second");
}

/* The set xk_trk_track and xk_trk_frame track with from now on: 0, or 1 once xk_trk_klt_second has declared it.  Nothing is queued */
extern "C" int xk_trk_klt_select(xk_trk *t, int set) {
  if (!t) return XK_EINVAL;
  xk_klt *k = t->klt;
  if (!k) return fail(t->h, XK_EINVAL, "xk_trk_klt_select: before xk_trk_klt_setup");
  if (set != 0 && set != 1) return fail(t->h, XK_EINVAL, "xk_trk_klt_select: set is 0 or 1");
  if (set == 1 && !k->has_second) return fail(t->h, XK_EINVAL, "xk_trk_klt_select: no second set (xk_trk_klt_second)");
  k->sel = set;
  return XK_OK;
}

/* the selected set, -1 before xk_trk_klt_setup */
extern "C" int xk_trk_klt_selected(xk_trk *t) { return (t && t->klt) ? t->klt->sel : -1; }

/* levels of rule 1 of the first set (the pyramid has levels + 1 images), -1 before xk_trk_klt_setup */
extern "C" int xk_trk_klt_levels(xk_trk *t) { return (t && t->klt) ? t->klt->levels : -1; }

/* levels of either set, -1 before xk_trk_klt_setup, for another value than 0 or 1 and for a second set that was not declared */
extern "C" int xk_trk_klt_levels_of(xk_trk *t, int set) {
  if (!t || !t->klt || (set != 0 && set != 1) || (set == 1 && !t->klt->has_second)) return -1;
  return set ? t->klt->levels2 : t->klt->levels;
}

// Levels 1 ... of a slot from its level 0, and the Scharr derivatives of every level.
static int klt_pyramid(xk_handle *h, const xk_klt *k, const XkKltPyr &P) {
  for (int l = 0; l <= k->deep; ++l) {
    const XkKltLevel &L = P.lv[l];
    if (l > 0) {
      const XkKltLevel &S = P.lv[l - 1];
      hipLaunchKernelGGL(xk_klt_pyrdown, dim3((L.w + XK_KLT_PD_TW - 1) / XK_KLT_PD_TW, (L.h + XK_KLT_PD_TH - 1) / XK_KLT_PD_TH), dim3(256), 0,
                         h->stream, S.img, S.w, S.h, S.pitch, L.img, L.w, L.h, L.pitch);
    }
    hipLaunchKernelGGL(xk_klt_scharr, dim3((L.w + 63) / 64, (L.h + 3) / 4), dim3(256), 0, h->stream, L.img, L.w, L.h, L.pitch, L.dx, L.dy);
  }
  return launched(h, "pyramid launch");
}

// The push behind xk_trk_push_image and xk_trk_frame: the arguments are checked and the device is set.
static int trk_push(xk_trk *t, const unsigned char *img, int stride) {
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  const int s = k->cur ^ 1;
  const XkKltPyr &P = k->slot[s];
  const XkKltPyr &B = photo_raw_slot(k, s);                                  // where the pyramid is built: the raw plane with a photo setup
  const size_t pitch0 = (size_t)P.lv[0].pitch;
  if (k->orb) k->orb->blurred[s] = 0;                                        // (the other slot's blur stays with its slot)
  if (k->pushed > 0) HIPCHK(h, hipEventSynchronize(k->img_copied));          // the staging is free again
  for (int y = 0; y < k->height; ++y) memcpy(k->h_img + y * pitch0, img + (size_t)y * stride, (size_t)k->width);
  HIPCHK(h, hipMemcpyAsync(B.lv[0].img, k->h_img, pitch0 * k->height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(k->img_copied, h->stream));
  XKCHK(klt_pyramid(h, k, B));
  if (k->photo) HIPCHK(h, hipMemcpyAsync(P.lv[0].img, B.lv[0].img, k->slot_bytes, hipMemcpyDeviceToDevice, h->stream));   // raw -> working
  k->cur = s;
  if (k->pushed < 2) ++k->pushed;
  return XK_OK;
}

/* previous_img_ = current_img.clone() (tracker.cpp:302) and the pyramid cv::calcOpticalFlowPyrLK builds of the new image */
extern "C" int xk_trk_push_image(xk_trk *t, const unsigned char *img, int stride) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_push_image: before xk_trk_klt_setup");
  if (!img || stride < k->width) return fail(h, XK_EINVAL, "xk_trk_push_image: null image or stride below the width");
  HIPCHK(h, hipSetDevice(h->device));
  XKCHK(trk_push(t, img, stride));
  if (k->frm) k->frm->n_res = -1;                                          // (the resident list belongs to an image that is no longer the previous one)
  return XK_OK;
}

// The kept pairs in a tracking's result block for n points: cur_xy [n][2] | min_eig [n] | kept pairs | status [n].
static XkKeptPairs klt_kept_at(unsigned char *d_res, int n) { return xk_kept_pairs((double *)d_res + 3 * (size_t)n, n); }

static XkKltSet klt_set(const xk_klt *k, int set) {
  return set ? XkKltSet{k->levels2, k->win_w2, k->win_h2, k->min_eig_thr2} : XkKltSet{k->levels, k->win_w, k->win_h, k->min_eig_thr};
}

// The tracking of the n points at d_pts from pyramid `prev` to `cur`, queued: the result block (klt_res_bytes(n)) goes to d_res.  With
// parameter set `set` (0 or 1) the host chose; with second_on (and a second set declared) the kernel takes set 1 where *second_on is not 0
// when it runs and set 0 otherwise, whatever `set` says.
static int klt_queue_track(xk_handle *h, const xk_klt *k, int set, const int *second_on, const XkKltPyr &prev, const XkKltPyr &cur,
                           const float *d_pts, unsigned char *d_res, int n, XkKltArgs &a, const int *n_dev = nullptr) {
  a = XkKltArgs{};
  a.n_dev = n_dev;                                                // (then n is the bound the grid and the block are sized by)
  a.prev = prev; a.cur = cur;
  if (second_on && k->has_second) { a.set[0] = klt_set(k, 0); a.set[1] = klt_set(k, 1); a.second_on = second_on; }
  else a.set[0] = a.set[1] = klt_set(k, set);
  a.n = n; a.max_iter = k->max_iter;
  a.eps2 = k->eps * k->eps;
  a.pts = d_pts;
  a.cur_xy = (double *)d_res; a.min_eig = a.cur_xy + 2 * (size_t)n;
  a.kept = klt_kept_at(d_res, n);
  a.status = xk_kept_pairs_end(a.kept, n);
  hipLaunchKernelGGL(xk_klt_track, dim3((n + XK_KLT_WAVES - 1) / XK_KLT_WAVES), dim3(64 * XK_KLT_WAVES), 0, h->stream, a);
  hipLaunchKernelGGL(xk_klt_compact, dim3(1), dim3(256), 0, h->stream, a);
  return launched(h, "feature tracking launch");
}

/* Tracker::featureTracking (tracker.cpp:623-690): cv::calcOpticalFlowPyrLK from the previous image to the current one, then the
 * pairs that were tracked and stayed inside the frame */
extern "C" int xk_trk_track(xk_trk *t, const float *prev_xy, int n, double *cur_xy, unsigned char *status, double *min_eig, int *keep_idx,
                            double *kept_prev_xy, double *kept_cur_xy, int *n_kept) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_track: before xk_trk_klt_setup");
  if (n < 0 || !cur_xy || !status || !min_eig || !keep_idx || !kept_prev_xy || !kept_cur_xy || !n_kept || (n > 0 && !prev_xy))
    return fail(h, XK_EINVAL, "xk_trk_track: null argument or negative n");
  if (k->pushed < 2) return fail(h, XK_EINVAL, "xk_trk_track: fewer than two images pushed");
  if (n > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_track: more features than max_matches");
  *n_kept = 0;
  if (n == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  memcpy(k->blk.h, prev_xy, sizeof(float) * 2 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync(k->d_pts, k->blk.h, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  XkKltArgs a;
  XKCHK(klt_queue_track(h, k, k->sel, nullptr, k->slot[k->cur ^ 1], k->slot[k->cur], k->d_pts, k->d_res, n, a));
  const unsigned char *r = k->h_res;
  HIPCHK(h, hipMemcpyAsync(k->h_res, k->d_res, klt_res_bytes(n), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  XKCHK(kept_pairs_out(h, "xk_trk_track", a.kept, k->d_res, r, n, keep_idx, kept_prev_xy, kept_cur_xy, n_kept));
  memcpy(cur_xy, r, sizeof(double) * 2 * (size_t)n);
  memcpy(min_eig, r + ((unsigned char *)a.min_eig - k->d_res), sizeof(double) * (size_t)n);
  memcpy(status, r + (a.status - k->d_res), (size_t)n);
  return XK_OK;
}

/* One pyramid level of the previous (which = 0) or the current (1) image as the device holds it: straight copies */
extern "C" int xk_trk_klt_level(xk_trk *t, int which, int level, unsigned char *img, short *dIx, short *dIy, int *w, int *hgt) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  const int s = img_slot(t, "xk_trk_klt_level", which);
  if (s < 0) return XK_EINVAL;
  if (level < 0 || level > t->klt->deep) return fail(h, XK_EINVAL, "xk_trk_klt_level: no such level");
  HIPCHK(h, hipSetDevice(h->device));
  const XkKltLevel &L = t->klt->slot[s].lv[level];
  if (w) *w = L.w;
  if (hgt) *hgt = L.h;
  if (img) HIPCHK(h, hipMemcpy2DAsync(img, (size_t)L.w, L.img, (size_t)L.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, h->stream));
  if (dIx) HIPCHK(h, hipMemcpy2DAsync(dIx, 2 * (size_t)L.w, L.dx, 2 * (size_t)L.pitch, 2 * (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, h->stream));
  if (dIy) HIPCHK(h, hipMemcpy2DAsync(dIy, 2 * (size_t)L.w, L.dy, 2 * (size_t)L.pitch, 2 * (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// ---------------------------------------------------------------------------
// FAST detection and neighbourhood selection of new features (tracker.cpp:390-590), xk_fast.hip.h
// ---------------------------------------------------------------------------
static size_t det_res_bytes(int n) { return sizeof(int) * (4 + 3 * (size_t)n); }

/* The parameters of Tracker::featureDetection as Tracker holds them (tracker.h:245-255) and the device buffers of one detection */
extern "C" int xk_trk_detect_setup(xk_trk *t, int threshold, int non_max_supp, int block_half_length, int margin, int max_candidates) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_detect_setup: before xk_trk_klt_setup");
  if (threshold < 1 || threshold > 254) return fail(h, XK_EINVAL, "xk_trk_detect_setup: threshold outside 1...254");
  if (non_max_supp < 0 || non_max_supp > 1) return fail(h, XK_EINVAL, "xk_trk_detect_setup: non_max_supp is 0 or 1");
  if (block_half_length < 0 || block_half_length > 4096) return fail(h, XK_EINVAL, "xk_trk_detect_setup: block_half_length outside 0...4096");
  if (margin < 0 || margin > 4096) return fail(h, XK_EINVAL, "xk_trk_detect_setup: margin outside 0...4096");
  if (max_candidates < 1 || max_candidates > XK_FAST_MAX_CAND) return fail(h, XK_EINVAL, "xk_trk_detect_setup: max_candidates outside 1...32768");
  HIPCHK(h, hipSetDevice(h->device));
  xk_det *d = (xk_det *)calloc(1, sizeof(xk_det));
  if (!d) return XK_ENOMEM;
  d->threshold = threshold; d->nms = non_max_supp; d->b = block_half_length; d->margin = margin; d->max_candidates = max_candidates;
  d->n_cand = -1;
  d->key_cap = 64;
  while (d->key_cap < max_candidates) d->key_cap <<= 1;
  d->wpr = (k->width + 31) / 32;
  const size_t key_lds = sizeof(unsigned int) * (size_t)d->key_cap, mask_bytes = sizeof(unsigned int) * (size_t)d->wpr * k->height;
  const bool mask_in_lds = key_lds + mask_bytes <= XK_FAST_LDS_MAX;
  d->lds_bytes = key_lds + (mask_in_lds ? mask_bytes : 0);
  const size_t s_bytes = (size_t)k->slot[0].lv[0].pitch * k->height, keys_bytes = up16(sizeof(unsigned int) * (size_t)max_candidates);
  const size_t old_bytes = sizeof(double) * 2 * (size_t)t->max_matches, res_bytes = up16(det_res_bytes(t->max_matches));
  int rc = blk_alloc(h, d->blk, s_bytes + keys_bytes + 16 + old_bytes + res_bytes + (mask_in_lds ? 0 : mask_bytes), old_bytes + res_bytes,
                     "xk_trk_detect_setup");
  if (rc == XK_OK && hipFuncSetAttribute((const void *)xk_fast_select, hipFuncAttributeMaxDynamicSharedMemorySize, XK_FAST_LDS_MAX) != hipSuccess)
    rc = fail(h, XK_ENOMEM, "xk_trk_detect_setup: allocation failed");
  if (rc == XK_OK) {
    size_t off = 0;
    d->S = carve<unsigned char>(d->blk.d, off, s_bytes);
    d->keys = carve<unsigned int>(d->blk.d, off, keys_bytes);
    d->count = carve<int>(d->blk.d, off, sizeof(int));
    d->old_xy = carve<double>(d->blk.d, off, old_bytes);
    d->res = carve<int>(d->blk.d, off, res_bytes);
    d->mask_g = mask_in_lds ? nullptr : carve<unsigned int>(d->blk.d, off, mask_bytes);
    d->h_res = (int *)(d->blk.h + old_bytes);
  }
  XKCHK(setup_install(h, rc, "xk_trk_detect_setup", k->det, d));
  frame_drop(k);
  return XK_OK;
}

// Accepted points are pairwise more than b apart: at most ceil(W / (b + 1)) ceil(H / (b + 1)) of them come back, and at most max_matches.
static int det_cap(const xk_trk *t, const xk_det *d) {
  const long long bound = (long long)((t->klt->width + d->b) / (d->b + 1)) * ((t->klt->height + d->b) / (d->b + 1));
  return (int)std::min<long long>(bound, t->max_matches);
}

// The detection on level 0 of slot s, queued: the result block goes to res.  The old features are the n_old at old_xy or, with n_old_dev,
// the device's count of at most n_old; pred as XkFastArgs::pred; alt_threshold >= 0: the photometric frame's, which the device selects
// (fast_detection_delta_photo_ once the calibration is done).
static int det_queue(xk_trk *t, int s, int *res, const double *old_xy, int n_old, const int *n_old_dev, const int *pred, int alt_threshold) {
  xk_handle *h = t->h;
  xk_det *d = t->klt->det;
  const XkKltLevel &L = t->klt->slot[s].lv[0];
  XkFastArgs a{};
  a.img = L.img; a.w = L.w; a.h = L.h; a.pitch = L.pitch;
  a.S = d->S; a.keys = d->keys; a.count = d->count; a.mask_g = d->mask_g; a.key_cap = d->key_cap; a.wpr = d->wpr;
  a.old_xy = old_xy; a.n_old = n_old; a.n_old_dev = n_old_dev; a.pred = pred;
  a.threshold = d->threshold; a.nms = d->nms; a.b = d->b; a.margin = d->margin; a.max_candidates = d->max_candidates;
  a.max_matches = t->max_matches;
  a.res = res;
  if (alt_threshold >= 0) { a.alt_on = &t->klt->photo->st->done; a.alt_threshold = alt_threshold; }
  d->n_cand = -1;                                                   // (the score image and the keys are no longer those xk_trk_detect_stage hands out)
  hipLaunchKernelGGL(xk_fast_score, dim3((a.w + XK_FAST_TW - 1) / XK_FAST_TW, (a.h + XK_FAST_TH - 1) / XK_FAST_TH), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(xk_fast_candidates, dim3((a.w + 63) / 64, (a.h + 3) / 4), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(xk_fast_select, dim3(1), dim3(XK_FAST_SEL_T), d->lds_bytes, h->stream, a);
  return launched(h, "detection launch");
}

/* Tracker::featureDetection (tracker.cpp:390-590) on level 0 of the previous (which = 0) or the current (1) image */
extern "C" int xk_trk_detect(xk_trk *t, int which, const double *old_xy, int n_old, int *xy, int *score, int *n_found, int *n_candidates) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_det *d = sub_of(t, &xk_klt::det, "xk_trk_detect", "xk_trk_detect_setup");
  if (!d) return XK_EINVAL;
  if (!xy || !score || !n_found || !n_candidates || n_old < 0 || (n_old > 0 && !old_xy))
    return fail(h, XK_EINVAL, "xk_trk_detect: null argument or negative n_old");
  const int s = img_slot(t, "xk_trk_detect", which);
  if (s < 0) return XK_EINVAL;
  *n_found = 0; *n_candidates = 0;
  if (n_old > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_detect: more old features than max_matches");
  HIPCHK(h, hipSetDevice(h->device));
  if (n_old > 0) {
    memcpy(d->blk.h, old_xy, sizeof(double) * 2 * (size_t)n_old);
    HIPCHK(h, hipMemcpyAsync(d->old_xy, d->blk.h, sizeof(double) * 2 * (size_t)n_old, hipMemcpyHostToDevice, h->stream));
  }
  XKCHK(det_queue(t, s, d->res, d->old_xy, n_old, nullptr, nullptr, -1));
  const int cap = det_cap(t, d);
  const int *r = d->h_res;
  HIPCHK(h, hipMemcpyAsync(d->h_res, d->res, det_res_bytes(t->max_matches), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int found = r[0], cand = r[1];
  if (found < 0 || cand < 0 || (cand <= d->max_candidates && found > cand)) return fail(h, XK_EDEVICE, "xk_trk_detect: counts out of range");
  d->n_cand = cand;
  *n_found = found; *n_candidates = cand;
  if (cand > d->max_candidates) return fail(h, XK_ECAPACITY, "xk_trk_detect: more candidates than max_candidates");
  if (found > cap) return fail(h, XK_ECAPACITY, "xk_trk_detect: more features accepted than max_matches");
  memcpy(xy, r + 4, sizeof(int) * 2 * (size_t)found);
  memcpy(score, r + 4 + 2 * (size_t)t->max_matches, sizeof(int) * (size_t)found);
  return XK_OK;
}

/* What the last detection left: the score image and the sorted keys.  Straight copies */
extern "C" int xk_trk_detect_stage(xk_trk *t, unsigned char *scores, unsigned int *keys, int *n_candidates) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_det *d = sub_of(t, &xk_klt::det, "xk_trk_detect_stage", "xk_trk_detect_setup");
  if (!d) return XK_EINVAL;
  if (d->n_cand < 0) return fail(h, XK_EINVAL, "xk_trk_detect_stage: before a detection");
  HIPCHK(h, hipSetDevice(h->device));
  if (n_candidates) *n_candidates = d->n_cand;
  const XkKltLevel &L = t->klt->slot[0].lv[0];
  if (scores) HIPCHK(h, hipMemcpy2DAsync(scores, (size_t)L.w, d->S, (size_t)L.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, h->stream));
  if (keys && d->n_cand > 0 && d->n_cand <= d->max_candidates)
    HIPCHK(h, hipMemcpyAsync(keys, d->keys, sizeof(unsigned int) * (size_t)d->n_cand, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Rotated-BRIEF descriptors of keypoints (place_recognition.cpp:72-94, tracker.cpp:440-444), xk_orb.hip.h
// ---------------------------------------------------------------------------
// The default pattern: candidate row r takes values 4r ... 4r + 3 of the splitmix64 stream of seed "ORB" (value i =
// mix(seed + (i + 1) golden), as the RANSAC sampler's), each mapped to -15 ... 15 by the high word's product with 31; a row
// whose two points coincide is skipped; the first 256 accepted rows.
static void orb_default_pattern(signed char *p) {
  const unsigned long long seed = 0x4F5242ull;
  for (unsigned long long row = 0, got = 0; got < 256; ++row) {
    int c[4];
    for (int k = 0; k < 4; ++k) {
      const unsigned long long z = xk_ransac_mix(seed + (4 * row + k + 1) * 0x9E3779B97F4A7C15ull);
      c[k] = (int)(((z >> 32) * 31ull) >> 32) - XK_ORB_HALF;
    }
    if (c[0] == c[2] && c[1] == c[3]) continue;
    for (int k = 0; k < 4; ++k) p[4 * got + k] = (signed char)c[k];
    ++got;
  }
}

/* The parameters of cv::ORB::compute as PlaceRecognition holds them (place_recognition.cpp:72-94) and the device buffers of one call */
extern "C" int xk_trk_describe_setup(xk_trk *t, int orientation, double angle_deg, int edge, const signed char *pattern, int max_desc) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_describe_setup: before xk_trk_klt_setup");
  if (orientation < 0 || orientation > 1) return fail(h, XK_EINVAL, "xk_trk_describe_setup: orientation is 0 (fixed angle) or 1 (intensity centroid)");
  if (!std::isfinite(angle_deg)) return fail(h, XK_EINVAL, "xk_trk_describe_setup: angle_deg is not finite");
  if (edge < 25 || edge > 4096) return fail(h, XK_EINVAL, "xk_trk_describe_setup: edge outside 25...4096");
  if (max_desc < 1 || max_desc > XK_ORB_MAX_DESC) return fail(h, XK_EINVAL, "xk_trk_describe_setup: max_desc outside 1...32768");
  if (pattern)
    for (int i = 0; i < 256; ++i) {
      const signed char *r = pattern + 4 * i;
      for (int c = 0; c < 4; ++c)
        if (r[c] < -XK_ORB_HALF || r[c] > XK_ORB_HALF) return fail(h, XK_EINVAL, "xk_trk_describe_setup: a pattern coordinate outside -15...15");
      if (r[0] == r[2] && r[1] == r[3]) return fail(h, XK_EINVAL, "xk_trk_describe_setup: a pattern row whose two points coincide");
    }
  HIPCHK(h, hipSetDevice(h->device));
  xk_orb *o = (xk_orb *)calloc(1, sizeof(xk_orb));
  if (!o) return XK_ENOMEM;
  o->centroid = orientation; o->edge = edge; o->max_desc = max_desc;
  const double th = angle_deg * (M_PI / 180.0);
  o->A = (int)std::rint(16384.0 * std::cos(th)); o->B = (int)std::rint(16384.0 * std::sin(th));
  if (pattern) memcpy(o->h_pattern, pattern, sizeof o->h_pattern);
  else orb_default_pattern(o->h_pattern);
  const size_t g_bytes = (size_t)k->slot[0].lv[0].pitch * k->height;
  const size_t xy_bytes = up16(sizeof(int) * 2 * (size_t)max_desc), res_bytes = up16(xk_orb_res_bytes((size_t)max_desc));
  int rc = blk_alloc(h, o->blk, 2 * g_bytes + sizeof o->h_pattern + 2 * xy_bytes + res_bytes,
                     std::max(xy_bytes + res_bytes, sizeof o->h_pattern), "xk_trk_describe_setup");   // (the pattern goes up through the mirror)
  if (rc == XK_OK) {
    size_t off = 0;
    o->G[0] = carve<unsigned char>(o->blk.d, off, g_bytes);
    o->G[1] = carve<unsigned char>(o->blk.d, off, g_bytes);
    o->pattern = carve<signed char>(o->blk.d, off, sizeof o->h_pattern);
    o->xy = carve<int>(o->blk.d, off, xy_bytes);
    o->kept_xy = carve<int>(o->blk.d, off, xy_bytes);
    o->res = carve<int>(o->blk.d, off, res_bytes);
    o->h_res = o->blk.h + xy_bytes;
    memcpy(o->blk.h, o->h_pattern, sizeof o->h_pattern);
    if (hipMemcpyAsync(o->pattern, o->blk.h, sizeof o->h_pattern, hipMemcpyHostToDevice, h->stream) != hipSuccess)
      rc = fail(h, XK_ENOMEM, "xk_trk_describe_setup: allocation failed");
  }
  XKCHK(setup_install(h, rc, "xk_trk_describe_setup", k->orb, o));
  frame_drop(k);
  return XK_OK;
}

// The blur of slot s into G[s], queued unless G[s] holds it, under pred (as XkOrbArgs::pred) if given.  The rule of blurred[s]: an
// unpredicated blur sets the flag; a predicated one may not have run, the host cannot count on it, and the flag stays clear.
static int orb_queue_blur(xk_trk *t, int s, const int *pred, XkOrbArgs &a) {
  xk_orb *o = t->klt->orb;
  const XkKltLevel &L = t->klt->slot[s].lv[0];
  a = XkOrbArgs{};
  a.img = L.img; a.G = o->G[s]; a.w = L.w; a.h = L.h; a.pitch = L.pitch; a.pred = pred;
  if (o->blurred[s]) return XK_OK;
  hipLaunchKernelGGL(xk_orb_blur, dim3((a.w + XK_ORB_TW - 1) / XK_ORB_TW, (a.h + XK_ORB_TH - 1) / XK_ORB_TH), dim3(256), 0, t->h->stream, a);
  XKCHK(launched(t->h, "blur launch"));
  if (!pred) o->blurred[s] = 1;
  return XK_OK;
}

// The description on slot s of the n keypoints at xy (with n_dev, the device's count of at most n), queued: the blur if it is the slot's
// first since its push, the filter, the descriptors.  The result block (xk_orb_res_bytes(n)) goes to res.
static int orb_queue(xk_trk *t, int s, const int *xy, int *res, int n, const int *n_dev, const int *pred) {
  xk_handle *h = t->h;
  const xk_orb *o = t->klt->orb;
  XkOrbArgs a;
  XKCHK(orb_queue_blur(t, s, pred, a));
  a.edge = o->edge; a.centroid = o->centroid; a.A = o->A; a.B = o->B;
  a.pattern = o->pattern; a.xy = xy; a.kept_xy = o->kept_xy; a.res = res;
  a.n = n; a.n_dev = n_dev;
  hipLaunchKernelGGL(xk_orb_filter, dim3(1), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(xk_orb_describe, dim3(std::min((n + XK_ORB_WAVES - 1) / XK_ORB_WAVES, XK_ORB_MAX_GRID)), dim3(64 * XK_ORB_WAVES), 0,
                     h->stream, a);
  return launched(h, "description launch");
}

/* cv::ORB::compute(img, keypoints, descriptors) (place_recognition.cpp:72-94) on the previous (which = 0) or the current (1) image */
extern "C" int xk_trk_describe(xk_trk *t, int which, const int *xy, int n, unsigned char *desc, int *keep_idx, int *dir, int *moments,
                               int *n_kept) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_orb *o = sub_of(t, &xk_klt::orb, "xk_trk_describe", "xk_trk_describe_setup");
  if (!o) return XK_EINVAL;
  if (!desc || !keep_idx || !dir || !moments || !n_kept || n < 0 || (n > 0 && !xy)) return fail(h, XK_EINVAL, "xk_trk_describe: null argument or negative n");
  const int s = img_slot(t, "xk_trk_describe", which);
  if (s < 0) return XK_EINVAL;
  if (n > o->max_desc) return fail(h, XK_ECAPACITY, "xk_trk_describe: more keypoints than max_desc");
  *n_kept = 0;
  if (n == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  memcpy(o->blk.h, xy, sizeof(int) * 2 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync(o->xy, o->blk.h, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  XKCHK(orb_queue(t, s, o->xy, o->res, n, nullptr, nullptr));
  const unsigned char *r = o->h_res;
  HIPCHK(h, hipMemcpyAsync(o->h_res, o->res, xk_orb_res_bytes((size_t)n), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  XKCHK(kept_count_out(h, "xk_trk_describe", r, n, n_kept));
  const size_t kept = (size_t)*n_kept;
  const int *ri = (const int *)r;
  memcpy(keep_idx, ri + 4, sizeof(int) * (size_t)kept);
  memcpy(dir, ri + 4 + n, sizeof(int) * 2 * (size_t)kept);
  memcpy(moments, ri + 4 + 3 * (size_t)n, sizeof(int) * 2 * (size_t)kept);
  memcpy(desc, r + xk_orb_desc_off((size_t)n), 32 * (size_t)kept);
  return XK_OK;
}

/* The blurred image of a slot and the pattern in use.  Straight copies */
extern "C" int xk_trk_describe_stage(xk_trk *t, int which, unsigned char *blurred, signed char *pattern) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_orb *o = sub_of(t, &xk_klt::orb, "xk_trk_describe_stage", "xk_trk_describe_setup");
  if (!o) return XK_EINVAL;
  const int s = img_slot(t, "xk_trk_describe_stage", which);
  if (s < 0) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (pattern) HIPCHK(h, hipMemcpyAsync(pattern, o->pattern, sizeof o->h_pattern, hipMemcpyDeviceToHost, h->stream));   // (the kernels' copy)
  if (blurred) {
    XkOrbArgs a;
    XKCHK(orb_queue_blur(t, s, nullptr, a));
    HIPCHK(h, hipMemcpy2DAsync(blurred, (size_t)a.w, a.G, (size_t)a.pitch, (size_t)a.w, (size_t)a.h, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Photometric calibration of the images (tracker.cpp:761-877, irPhotoCalib.cpp), xk_photo.hip.h
// ---------------------------------------------------------------------------
// The state as a reset leaves it, queued through the pinned block: the caller waits.
static int photo_state_reset(xk_handle *h, xk_photo *p) {
  XkPhotoState *s = (XkPhotoState *)p->blk.h;
  memset(s, 0, sizeof *s);
  s->ring[0] = 1.0; s->ring[1] = 0.0;                                             // irPhotoCalib.cpp:25
  s->ring_n = 1;
  HIPCHK(h, hipMemcpyAsync(p->st, s, sizeof *s, hipMemcpyHostToDevice, h->stream));
  p->ring_n = 1; p->done = 0;
  memset(p->n_hyp, 0, sizeof p->n_hyp);
  return XK_OK;
}

/* The parameters of IRPhotoCalib and of Tracker::computeIntensity as Tracker holds them (tracker.h:366, irPhotoCalib.cpp:15-25), the
 * raw planes, the spatial map and the parameter ring */
extern "C" int xk_trk_photo_setup(xk_trk *t, int kernel_size, double epsilon_gap, double epsilon_base, int max_hyp) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_photo_setup: before xk_trk_klt_setup");
  if (kernel_size < 2 || kernel_size > 64) return fail(h, XK_EINVAL, "xk_trk_photo_setup: kernel_size outside 2...64");
  if (!(epsilon_gap >= 0.0 && epsilon_gap <= 1.0) || !(epsilon_base >= 0.0 && epsilon_base <= 1.0))
    return fail(h, XK_EINVAL, "xk_trk_photo_setup: epsilon_gap or epsilon_base outside [0, 1]");
  if (max_hyp < 1 || max_hyp > XK_PHOTO_MAX_HYP) return fail(h, XK_EINVAL, "xk_trk_photo_setup: max_hyp outside 1...4096");
  HIPCHK(h, hipSetDevice(h->device));
  xk_photo *p = (xk_photo *)calloc(1, sizeof(xk_photo));
  if (!p) return XK_ENOMEM;
  p->kernel_size = kernel_size; p->max_hyp = max_hyp; p->eps_gap = epsilon_gap; p->eps_base = epsilon_base;
  const size_t mm = (size_t)round_up(t->max_matches, 4), gm = XK_PHOTO_MAX_GROUPS * mm;
  const size_t ps_bytes = sizeof(float) * (size_t)k->slot[0].lv[0].pitch * k->height;
  const size_t sc_bytes = up16(xk_ransac_scratch_bytes<1>((size_t)max_hyp));
  // the i/o block, every piece a multiple of 16 bytes: state | value | sum, count | the tracking's result block | previous intensities,
  // previous points, pixels | o_hist, o_cur | off | frame_back
  const size_t io_bytes = up16(sizeof(XkPhotoState)) + 8 * mm + 2 * 4 * mm + up16(klt_res_bytes(t->max_matches)) + 3 * 8 * mm + 2 * 8 * gm + 64 + 64;
  int rc = blk_alloc(h, p->blk, 2 * k->slot_bytes + ps_bytes + io_bytes + XK_PHOTO_MAX_GROUPS * sc_bytes, io_bytes, "xk_trk_photo_setup");
  if (rc == XK_OK) {
    size_t off = 0;
    bool ok = true;
    for (int s = 0; s < 2; ++s) {
      p->raw[s] = k->slot[s];                                                           // the same layout at another base
      klt_place(p->raw[s], k->deep, carve<unsigned char>(p->blk.d, off, k->slot_bytes));
      // images pushed before this call are raw and working at once
      ok = ok && hipMemcpyAsync(p->raw[s].lv[0].img, k->slot[s].lv[0].img, k->slot_bytes, hipMemcpyDeviceToDevice, h->stream) == hipSuccess;
    }
    p->PS = carve<float>(p->blk.d, off, ps_bytes);
    unsigned char *io = p->d_io = carve<unsigned char>(p->blk.d, off, io_bytes);
    for (int g = 0; g < XK_PHOTO_MAX_GROUPS; ++g) p->sc[g] = xk_ransac_scratch<1>(carve<unsigned char>(p->blk.d, off, sc_bytes), (size_t)max_hyp);
    off = 0;
    p->st = carve<XkPhotoState>(io, off, sizeof(XkPhotoState));
    p->value = carve<double>(io, off, 8 * mm); p->sum = carve<int>(io, off, 4 * mm); p->count = carve<int>(io, off, 4 * mm);
    p->klt_res = carve<unsigned char>(io, off, klt_res_bytes(t->max_matches));
    p->prev_int = carve<double>(io, off, 8 * mm); p->pts = carve<float>(io, off, 8 * mm); p->ixy = carve<int>(io, off, 8 * mm);
    p->o_hist = carve<double>(io, off, 8 * gm); p->o_cur = carve<double>(io, off, 8 * gm);
    p->off = carve<int>(io, off, 64); p->frame_back = carve<int>(io, off, 64);
    if (!ok || photo_state_reset(h, p) != XK_OK) rc = fail(h, XK_ENOMEM, "xk_trk_photo_setup: allocation failed");
  }
  XKCHK(setup_install(h, rc, "xk_trk_photo_setup", k->photo, p));
  if (k->frm) {                                                    // (the photometric frame setup was made over the old photo setup)
    setup_free(k->frm->pf);
    k->frm->pf = nullptr;
  }
  return XK_OK;
}

// the pinned mirror of a device pointer into the i/o block
template <class T>
static T *photo_host(const xk_photo *p, const T *dev) { return (T *)(p->blk.h + ((const unsigned char *)dev - p->d_io)); }

static XkPhotoIntArgs photo_int_args(const xk_photo *p, const XkKltLevel &L, int n) {
  XkPhotoIntArgs a{};
  a.img = L.img; a.w = L.w; a.h = L.h; a.pitch = L.pitch; a.hk = p->kernel_size / 2;
  a.xy = p->ixy; a.n = n; a.value = p->value; a.sum = p->sum; a.count = p->count;
  return a;
}

/* Tracker::computeIntensity (tracker.cpp:860-877) of n pixels on level 0 of a slot's raw (plane = 0) or working (1) image */
extern "C" int xk_trk_photo_intensity(xk_trk *t, int which, int plane, const int *xy, int n, double *value, int *sum, int *count) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_intensity", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  xk_klt *k = t->klt;
  if (n < 0 || !value || !sum || !count || (n > 0 && !xy)) return fail(h, XK_EINVAL, "xk_trk_photo_intensity: null argument or negative n");
  if (plane < 0 || plane > 1) return fail(h, XK_EINVAL, "xk_trk_photo_intensity: plane is 0 or 1");
  const int s = img_slot(t, "xk_trk_photo_intensity", which);
  if (s < 0) return XK_EINVAL;
  if (n > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_photo_intensity: more points than max_matches");
  if (n == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const XkPhotoIntArgs a = photo_int_args(p, (plane == 0 ? p->raw[s] : k->slot[s]).lv[0], n);
  memcpy(photo_host(p, p->ixy), xy, sizeof(int) * 2 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync(p->ixy, photo_host(p, p->ixy), sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_photo_intensity, dim3((n + XK_PHOTO_WAVES - 1) / XK_PHOTO_WAVES), dim3(64 * XK_PHOTO_WAVES), 0, h->stream, a);
  XKCHK(launched(h, "intensity launch"));
  const size_t out_bytes = (size_t)((unsigned char *)p->klt_res - (unsigned char *)p->value);     // value | sum | count
  HIPCHK(h, hipMemcpyAsync(photo_host(p, p->value), p->value, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(value, photo_host(p, p->value), sizeof(double) * (size_t)n);
  memcpy(sum, photo_host(p, p->sum), sizeof(int) * (size_t)n);
  memcpy(count, photo_host(p, p->count), sizeof(int) * (size_t)n);
  return XK_OK;
}

// The solve, score and refit of group g and, after the last group, the chain: queued, no wait.
static int photo_queue_gains(xk_handle *h, xk_photo *p, XkPhotoGainArgs &a) {
  for (int g = 0; g < a.G; ++g) {
    a.g = g; a.sc = p->sc[g];
    hipLaunchKernelGGL(xk_photo_solve, dim3((a.n_hyp + XK_PHOTO_SOLVE_T - 1) / XK_PHOTO_SOLVE_T), dim3(XK_PHOTO_SOLVE_T), 0, h->stream, a);
    hipLaunchKernelGGL(xk_photo_score, dim3(a.n_hyp), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(xk_photo_refit, dim3(1), dim3(256), 0, h->stream, a);
  }
  hipLaunchKernelGGL(xk_photo_chain, dim3(1), dim3(64), 0, h->stream, a);
  return launched(h, "gain estimation launch");
}

static XkPhotoGainArgs photo_gain_args(const xk_photo *p, int G, int n_hyp, unsigned long seed, int per_frame) {
  XkPhotoGainArgs a{};
  a.o_hist = p->o_hist; a.o_cur = per_frame ? p->value : p->o_cur;
  a.off = p->off; a.frame_back = p->frame_back;
  a.G = G; a.n_hyp = n_hyp; a.per_frame = per_frame; a.seed = (unsigned long long)seed;
  a.eps_gap = p->eps_gap; a.eps_base = p->eps_base; a.st = p->st;
  return a;
}

// the state out of the pinned block after a wait
static int photo_state_out(xk_handle *h, xk_photo *p, int G, double *a_rel, double *b_rel, int *support, double *frame_ab) {
  const XkPhotoState *s = (const XkPhotoState *)p->blk.h;
  if (s->ring_n < 1 || s->ring_n > XK_PHOTO_RING) return fail(h, XK_EDEVICE, "photometric state: ring size out of range");
  p->ring_n = s->ring_n; p->done = s->done;
  if (a_rel) memcpy(a_rel, s->a_rel, sizeof(double) * (size_t)G);
  if (b_rel) memcpy(b_rel, s->b_rel, sizeof(double) * (size_t)G);
  if (support) memcpy(support, s->support, sizeof(int) * (size_t)G);
  if (frame_ab) memcpy(frame_ab, s->frame_ab, sizeof s->frame_ab);
  return XK_OK;
}

/* IRPhotoCalib::ProcessCurrentFrame (irPhotoCalib.cpp:95-160, :212-218) with EstimateGainsRansac (:221-312) per group */
extern "C" int xk_trk_photo_gains(xk_trk *t, int G, const int *off, const double *o_hist, const double *o_cur, const int *frame_back, int n_hyp,
                                  unsigned long seed, double *a_rel, double *b_rel, int *support, double *frame_ab) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_gains", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  if (G < 1 || G > XK_PHOTO_MAX_GROUPS) return fail(h, XK_EINVAL, "xk_trk_photo_gains: G outside 1...14");
  if (!off || !frame_back || !a_rel || !b_rel || !support || !frame_ab) return fail(h, XK_EINVAL, "xk_trk_photo_gains: null argument");
  if (n_hyp < 1 || n_hyp > p->max_hyp) return fail(h, XK_EINVAL, "xk_trk_photo_gains: n_hyp outside 1...max_hyp");
  if (off[0] != 0) return fail(h, XK_EINVAL, "xk_trk_photo_gains: off[0] is not 0");
  for (int g = 0; g < G; ++g) {
    if (off[g + 1] < off[g]) return fail(h, XK_EINVAL, "xk_trk_photo_gains: off is not ascending");
    if (off[g + 1] - off[g] > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_photo_gains: a group of more points than max_matches");
    if (frame_back[g] < 1 || frame_back[g] > p->ring_n) return fail(h, XK_EINVAL, "xk_trk_photo_gains: frame_back outside 1...the ring's size");
  }
  const int total = off[G];
  if (total > 0 && (!o_hist || !o_cur)) return fail(h, XK_EINVAL, "xk_trk_photo_gains: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  // one copy in: o_hist | o_cur | off | frame_back are adjacent, the lists at their full stride
  memcpy(photo_host(p, p->o_hist), o_hist, sizeof(double) * (size_t)total);
  memcpy(photo_host(p, p->o_cur), o_cur, sizeof(double) * (size_t)total);
  memcpy(photo_host(p, p->off), off, sizeof(int) * (size_t)(G + 1));
  memcpy(photo_host(p, p->frame_back), frame_back, sizeof(int) * (size_t)G);
  const size_t in_at = (size_t)((unsigned char *)p->o_hist - p->d_io);
  HIPCHK(h, hipMemcpyAsync(p->o_hist, p->blk.h + in_at, p->blk.h_bytes - in_at, hipMemcpyHostToDevice, h->stream));
  XkPhotoGainArgs a = photo_gain_args(p, G, n_hyp, seed, 0);
  memset(p->n_hyp, 0, sizeof p->n_hyp);
  XKCHK(photo_queue_gains(h, p, a));
  HIPCHK(h, hipMemcpyAsync(p->blk.h, p->st, sizeof(XkPhotoState), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int g = 0; g < G; ++g) p->n_hyp[g] = off[g + 1] - off[g] > 4 ? n_hyp : 0;
  return photo_state_out(h, p, G, a_rel, b_rel, support, frame_ab);
}

/* What the last gain estimate left for hypotheses first ... first+count-1 of group g.  Straight copies */
extern "C" int xk_trk_photo_hypotheses(xk_trk *t, int g, int first, int count, double *ab, int *inliers) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_hypotheses", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  if (g < 0 || g >= XK_PHOTO_MAX_GROUPS) return fail(h, XK_EINVAL, "xk_trk_photo_hypotheses: no such group");
  if (first < 0 || count < 0) return fail(h, XK_EINVAL, "xk_trk_photo_hypotheses: negative range");
  if (first + (long)count > p->n_hyp[g]) return fail(h, XK_EINVAL, "xk_trk_photo_hypotheses: range outside the hypotheses of the last estimate");
  if (count == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const XkRansacScratch &s = p->sc[g];
  if (ab) HIPCHK(h, hipMemcpy2DAsync(ab, 2 * sizeof(double), s.cand + 9 * (size_t)first, 9 * sizeof(double), 2 * sizeof(double), (size_t)count,
                                    hipMemcpyDeviceToHost, h->stream));
  if (inliers) HIPCHK(h, hipMemcpyAsync(inliers, s.cnt + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

/* params_PT_ (irPhotoCalib.cpp:25, :213-218): the ring's pairs, oldest first.  A straight copy */
extern "C" int xk_trk_photo_params(xk_trk *t, double *a, double *b, int *count) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_params", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  if (!count) return fail(h, XK_EINVAL, "xk_trk_photo_params: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(p->blk.h, p->st, sizeof(XkPhotoState), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const XkPhotoState *s = (const XkPhotoState *)p->blk.h;
  if (s->ring_n < 1 || s->ring_n > XK_PHOTO_RING) return fail(h, XK_EDEVICE, "xk_trk_photo_params: ring size out of range");
  *count = s->ring_n;
  for (int i = 0; i < s->ring_n; ++i) {
    if (a) a[i] = s->ring[2 * i];
    if (b) b[i] = s->ring[2 * i + 1];
  }
  return XK_OK;
}

/* The ring back to its one entry (1, 0), no gains estimated yet */
extern "C" int xk_trk_photo_reset(xk_trk *t) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_reset", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));                                       // (the pinned block is free)
  XKCHK(photo_state_reset(h, p));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

/* params_PS_ (irPhotoCalib.cpp:36): the caller's spatial map, float32 [height][width]; NULL: zeros */
extern "C" int xk_trk_photo_set_spatial(xk_trk *t, const float *ps) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_set_spatial", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  xk_klt *k = t->klt;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t pitch = sizeof(float) * (size_t)k->slot[0].lv[0].pitch;
  if (ps) HIPCHK(h, hipMemcpy2DAsync(p->PS, pitch, ps, sizeof(float) * (size_t)k->width, sizeof(float) * (size_t)k->width, (size_t)k->height,
                                    hipMemcpyHostToDevice, h->stream));
  else HIPCHK(h, hipMemsetAsync(p->PS, 0, pitch * k->height, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));                                       // (the caller's array is free again)
  return XK_OK;
}

// The correction of slot s queued: level 0 of the working plane from the raw one, then its pyramid and derivatives.
static int photo_queue_correct(xk_handle *h, xk_klt *k, int s, int per_frame) {
  xk_photo *p = k->photo;
  const XkKltLevel &R = p->raw[s].lv[0], &W = k->slot[s].lv[0];
  XkPhotoCorrectArgs a{};
  a.raw = R.img; a.out = W.img; a.PS = p->PS; a.w = W.w; a.h = W.h; a.pitch = W.pitch; a.per_frame = per_frame; a.st = p->st;
  const int threads = (W.pitch / 16) * W.h;
  hipLaunchKernelGGL(xk_photo_correct, dim3((threads + 255) / 256), dim3(256), 0, h->stream, a);
  XKCHK(launched(h, "correction launch"));
  if (k->orb) k->orb->blurred[s] = 0;
  return klt_pyramid(h, k, k->slot[s]);
}

/* IRPhotoCalib::getCorrectedImage (irPhotoCalib.cpp:442-472) of the previous (which = 0) or the current (1) image, with the ring's
 * last pair */
extern "C" int xk_trk_photo_correct(xk_trk *t, int which) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_correct", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  const int s = img_slot(t, "xk_trk_photo_correct", which);
  if (s < 0) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  return photo_queue_correct(h, t->klt, s, 0);
}

/* Level 0 of a slot's raw plane: the image as pushed.  A straight copy */
extern "C" int xk_trk_photo_raw(xk_trk *t, int which, unsigned char *img) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_raw", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  if (!img) return fail(h, XK_EINVAL, "xk_trk_photo_raw: null argument");
  const int s = img_slot(t, "xk_trk_photo_raw", which);
  if (s < 0) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const XkKltLevel &L = p->raw[s].lv[0];
  HIPCHK(h, hipMemcpy2DAsync(img, (size_t)L.w, L.img, (size_t)L.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// What every launch of xk_photo_sp_accumulate shares: the grid, the caps, the lists it appends to.  The caller adds the points.
static XkPspAccArgs psp_acc_args(const xk_photo *p, const xk_psp *s, int G) {
  XkPspAccArgs a{};
  a.g = s->g; a.max_count = s->max_count; a.max_rows = s->max_rows; a.thr = (double)s->thr;
  a.G = G; a.ring = p->st;
  a.count = s->count; a.coverage = s->coverage; a.sid_hist = s->sid_hist; a.sid_cur = s->sid_cur; a.b = s->b; a.st = s->st;
  return a;
}

// calibrateImage of n >= 4 features up to the correction, queued: the tracking of the device's points d_pts between the RAW planes (its
// result block is p->klt_res, its kept pairs come back in `kept`), the kept features' previous intensities out of prev_int and their
// pixels gathered, their intensities in the raw current plane, the gains, and the rows of a spatial setup that is still accumulating.
static int photo_queue_calibrate(xk_trk *t, const float *d_pts, const double *prev_int, int n, int n_hyp, unsigned long seed, XkKeptPairs &kept) {
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  xk_photo *p = k->photo;
  XkKltArgs a;
  XKCHK(klt_queue_track(h, k, 0, nullptr, p->raw[k->cur ^ 1], p->raw[k->cur], d_pts, p->klt_res, n, a));    // always the first set (tracker.cpp:784-787)
  kept = a.kept;
  XkPhotoGatherArgs ga{};
  ga.kept = kept; ga.prev_intensity = prev_int; ga.ixy = p->ixy; ga.o_hist = p->o_hist; ga.off = p->off; ga.frame_back = p->frame_back;
  hipLaunchKernelGGL(xk_photo_gather, dim3((n + 255) / 256), dim3(256), 0, h->stream, ga);
  XkPhotoIntArgs ia = photo_int_args(p, p->raw[k->cur].lv[0], n);
  ia.n_dev = kept.res;
  hipLaunchKernelGGL(xk_photo_intensity, dim3((n + XK_PHOTO_WAVES - 1) / XK_PHOTO_WAVES), dim3(64 * XK_PHOTO_WAVES), 0, h->stream, ia);
  XKCHK(launched(h, "calibration launch"));
  XkPhotoGainArgs g = photo_gain_args(p, 1, n_hyp, seed, 1);
  XKCHK(photo_queue_gains(h, p, g));
  if (p->sp && p->sp->state != XK_PSP_ESTIMATED) {               // the spatial rows of this frame, from the lists already on the device
    XkPspAccArgs sa = psp_acc_args(p, p->sp, 1);
    sa.prev_f = d_pts; sa.keep_idx = kept.keep_idx; sa.pix_cur = p->ixy; sa.o_hist = p->o_hist; sa.o_cur = p->value;
    sa.off = p->off; sa.frame_back = p->frame_back; sa.per_frame = 1;
    hipLaunchKernelGGL(xk_photo_sp_accumulate, dim3(1), dim3(64), 0, h->stream, sa);
  }
  return XK_OK;
}

/* Tracker::calibrateImage (tracker.cpp:761-858): track the previous features between the RAW images, their intensities in the
 * current one, the gain estimate against the previous intensities, the correction of the current image */
extern "C" int xk_trk_photo_calibrate(xk_trk *t, const float *prev_xy, const double *prev_intensity, int n, int n_hyp, unsigned long seed,
                                      int *keep_idx, double *intensity, int *sum, int *count, int *n_kept, double *a_rel, double *b_rel,
                                      int *support, double *frame_ab, int *estimated) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_calibrate", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  xk_klt *k = t->klt;
  if (n < 0 || !keep_idx || !intensity || !sum || !count || !n_kept || !a_rel || !b_rel || !support || !frame_ab || !estimated ||
      (n > 0 && (!prev_xy || !prev_intensity)))
    return fail(h, XK_EINVAL, "xk_trk_photo_calibrate: null argument or negative n");
  if (n_hyp < 1 || n_hyp > p->max_hyp) return fail(h, XK_EINVAL, "xk_trk_photo_calibrate: n_hyp outside 1...max_hyp");
  if (k->pushed < 2) return fail(h, XK_EINVAL, "xk_trk_photo_calibrate: fewer than two images pushed");
  if (n > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_photo_calibrate: more features than max_matches");
  *n_kept = 0; *estimated = 0;
  *a_rel = 1.0; *b_rel = 0.0; *support = 0;
  memset(frame_ab, 0, 4 * sizeof(double));
  memset(p->n_hyp, 0, sizeof p->n_hyp);
  HIPCHK(h, hipSetDevice(h->device));
  if (n < 4) {                                                   // tracker.cpp:763: corrected only after an earlier estimate
    if (!p->done) return XK_OK;
    XKCHK(photo_queue_correct(h, k, k->cur, 1));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return XK_OK;
  }
  // one copy in: previous intensities | previous points
  memcpy(photo_host(p, p->prev_int), prev_intensity, sizeof(double) * (size_t)n);
  memcpy(photo_host(p, p->pts), prev_xy, sizeof(float) * 2 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync(p->prev_int, photo_host(p, p->prev_int), (size_t)((unsigned char *)p->ixy - (unsigned char *)p->prev_int),
                           hipMemcpyHostToDevice, h->stream));
  XkKeptPairs kp;
  XKCHK(photo_queue_calibrate(t, p->pts, p->prev_int, n, n_hyp, seed, kp));
  XKCHK(photo_queue_correct(h, k, k->cur, 1));
  // one copy out: state | value | sum | count | the tracking's result block
  const size_t out_bytes = (size_t)(p->klt_res - p->d_io) + klt_res_bytes(n);
  HIPCHK(h, hipMemcpyAsync(p->blk.h, p->d_io, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const unsigned char *r = photo_host(p, p->klt_res);
  XKCHK(kept_count_out(h, "xk_trk_photo_calibrate", r + ((unsigned char *)kp.res - p->klt_res), n, n_kept));
  const int kept = *n_kept;
  memcpy(keep_idx, r + ((unsigned char *)kp.keep_idx - p->klt_res), sizeof(int) * (size_t)kept);
  memcpy(intensity, photo_host(p, p->value), sizeof(double) * (size_t)kept);
  memcpy(sum, photo_host(p, p->sum), sizeof(int) * (size_t)kept);
  memcpy(count, photo_host(p, p->count), sizeof(int) * (size_t)kept);
  const XkPhotoState *s = (const XkPhotoState *)p->blk.h;
  *estimated = s->estimated;
  if (kept > 4) p->n_hyp[0] = n_hyp;
  if (!s->estimated) return photo_state_out(h, p, 0, nullptr, nullptr, nullptr, nullptr);
  return photo_state_out(h, p, 1, a_rel, b_rel, support, frame_ab);
}

// ---------------------------------------------------------------------------
// The spatial photometric map estimated on the device (irPhotoCalib.cpp:162-210, :314-420), xk_photo_spatial.hip.h
// ---------------------------------------------------------------------------
#define XK_PSP_BATCH 32            // iterations queued between two looks at the done flag
#define XK_PSP_WAIT_S 20.0         // the bound of every host wait of the estimate

static double psp_now() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// The state block into its pinned mirror and a bounded wait for it: a batch that does not come back is XK_EDEVICE, never a spin.
static int psp_fetch(xk_handle *h, xk_psp *s, const char *who) {
  HIPCHK(h, hipMemcpyAsync(s->blk.h, s->st, sizeof(XkPspState), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(s->batch, h->stream));
  const double until = psp_now() + XK_PSP_WAIT_S;
  for (;;) {
    const hipError_t e = hipEventQuery(s->batch);
    if (e == hipSuccess) return XK_OK;
    if (e != hipErrorNotReady) return fail(h, XK_EDEVICE, who, e);
    if (psp_now() > until) return fail_at(h, XK_EDEVICE, who, "a batch of launches did not come back");
    sched_yield();
  }
}

static const XkPspState *psp_host(const xk_psp *s) { return (const XkPspState *)s->blk.h; }

// counts, coverage, rows and the state back to empty: queued, the caller waits
static int psp_queue_reset(xk_handle *h, xk_psp *s) {
  HIPCHK(h, hipMemsetAsync(s->count, 0, sizeof(int) * (size_t)s->g.cells, h->stream));
  HIPCHK(h, hipMemsetAsync(s->coverage, 0, s->cov_bytes, h->stream));
  HIPCHK(h, hipMemsetAsync(s->st, 0, sizeof(XkPspState), h->stream));
  s->state = XK_PSP_ACCUMULATING;
  s->staged_n = -1;
  return XK_OK;
}

/* temporal_params_div, spatial_params_thr, SP_max_correscount_ and the GP's hyperparameters (irPhotoCalib.cpp:15-55) */
extern "C" int xk_trk_photo_spatial_setup(xk_trk *t, int div, double coverage_thr, int max_count, int max_rows, double gp_length,
                                          double gp_sigma_f, double gp_sigma_n) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_spatial_setup", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  xk_klt *k = t->klt;
  if (div < 2 || div > 256) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_setup: div outside 2...256");
  const int cw = k->width / div, ch = k->height / div;
  if ((long)cw * ch < 2) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_setup: fewer than 2 cells");
  if (!std::isfinite(coverage_thr) || !std::isfinite(gp_length) || !std::isfinite(gp_sigma_f) || !std::isfinite(gp_sigma_n))
    return fail(h, XK_EINVAL, "xk_trk_photo_spatial_setup: a parameter is not finite");
  if (max_count < 1 || max_rows < 1) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_setup: max_count or max_rows < 1");
  if (!((float)gp_length > 0.f) || !((float)gp_sigma_f > 0.f) || !((float)gp_sigma_n > 0.f))
    return fail(h, XK_EINVAL, "xk_trk_photo_spatial_setup: a hyperparameter <= 0");
  HIPCHK(h, hipSetDevice(h->device));
  xk_psp *s = (xk_psp *)calloc(1, sizeof(xk_psp));
  if (!s) return XK_ENOMEM;
  s->g = XkPspGrid{k->width, k->height, div, cw, ch, cw * ch};
  s->max_count = max_count; s->max_rows = max_rows;
  s->n_max = std::min(s->g.cells, XK_PSP_NMAX); s->ld = round_up(s->n_max, 2);
  s->thr = (float)coverage_thr; s->gp_l = (float)gp_length; s->gp_sf = (float)gp_sigma_f; s->gp_sn = (float)gp_sigma_n;
  const size_t cells = (size_t)s->g.cells, nm = (size_t)s->n_max, mat = sizeof(double) * nm * (size_t)s->ld;
  const size_t gm = XK_PHOTO_MAX_GROUPS * (size_t)round_up(t->max_matches, 4);
  const size_t ps_bytes = sizeof(float) * (size_t)k->slot[0].lv[0].pitch * k->height;
  s->cov_bytes = up16(cells);
  s->in_bytes = 4 * 8 * gm + 128;
  const size_t st_bytes = up16(sizeof(XkPspState));
  const size_t slots = (nm + XK_PSP_MV_ROWS - 1) / XK_PSP_MV_ROWS;
  const size_t d_bytes = up16(4 * cells) + s->cov_bytes + 2 * up16(4 * (size_t)max_rows) + up16(8 * (size_t)max_rows) + up16(4 * cells) +
                         2 * up16(4 * nm) + 2 * up16(mat) + 8 * up16(8 * nm) + up16(8 * slots) + up16(4 * cells) + up16(ps_bytes) + st_bytes +
                         s->in_bytes;
  int rc = blk_alloc(h, s->blk, d_bytes, st_bytes + s->in_bytes, "xk_trk_photo_spatial_setup");
  if (rc == XK_OK) {
    size_t off = 0;
    unsigned char *d = s->blk.d;
    s->count = carve<int>(d, off, 4 * cells); s->coverage = carve<unsigned char>(d, off, s->cov_bytes);
    s->sid_hist = carve<int>(d, off, 4 * (size_t)max_rows); s->sid_cur = carve<int>(d, off, 4 * (size_t)max_rows);
    s->b = carve<double>(d, off, 8 * (size_t)max_rows);
    s->var_of_cell = carve<int>(d, off, 4 * cells); s->cell_of_var = carve<int>(d, off, 4 * nm); s->deg = carve<int>(d, off, 4 * nm);
    s->L = carve<double>(d, off, mat); s->K = carve<double>(d, off, mat);
    s->c = carve<double>(d, off, 8 * nm); s->x = carve<double>(d, off, 8 * nm); s->alpha = carve<double>(d, off, 8 * nm);
    s->r = carve<double>(d, off, 8 * nm); s->p = carve<double>(d, off, 8 * nm); s->q = carve<double>(d, off, 8 * nm);
    s->diag_l = carve<double>(d, off, 8 * nm); s->diag_k = carve<double>(d, off, 8 * nm);
    s->partial = carve<double>(d, off, 8 * slots);
    s->coarse = carve<float>(d, off, 4 * cells); s->ps = carve<float>(d, off, ps_bytes);
    s->st = carve<XkPspState>(d, off, sizeof(XkPspState));
    s->d_in = carve<unsigned char>(d, off, s->in_bytes);
    s->staged_n = -1;
    if (hipEventCreateWithFlags(&s->batch, hipEventDisableTiming) != hipSuccess) rc = fail(h, XK_ENOMEM, "xk_trk_photo_spatial_setup: allocation failed");
  }
  return setup_install(h, rc, "xk_trk_photo_spatial_setup", p->sp, s);       // (blk_alloc zeroed the block: accumulating, no rows)
}

// the spatial setup of entry `who`, or nullptr after fail(XK_EINVAL)
static xk_psp *psp_of(xk_trk *t, const char *who) {
  xk_photo *p = sub_of(t, &xk_klt::photo, who, "xk_trk_photo_setup");
  if (!p) return nullptr;
  if (!p->sp) fail_at(t->h, XK_EINVAL, who, "before xk_trk_photo_spatial_setup");
  return p->sp;
}

/* The spatial part of one IRPhotoCalib::ProcessCurrentFrame (irPhotoCalib.cpp:162-198) against the ring as it stands */
extern "C" int xk_trk_photo_spatial_add(xk_trk *t, int G, const int *off, const int *pix_hist, const int *pix_cur, const double *o_hist,
                                        const double *o_cur, const int *frame_back) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_psp *s = psp_of(t, "xk_trk_photo_spatial_add");
  if (!s) return XK_EINVAL;
  xk_photo *p = t->klt->photo;
  if (G < 1 || G > XK_PHOTO_MAX_GROUPS) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_add: G outside 1...14");
  if (!off || !frame_back) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_add: null argument");
  if (off[0] != 0) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_add: off[0] is not 0");
  for (int g = 0; g < G; ++g) {
    if (off[g + 1] < off[g]) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_add: off is not ascending");
    if (off[g + 1] - off[g] > t->max_matches) return fail(h, XK_ECAPACITY, "xk_trk_photo_spatial_add: a group of more points than max_matches");
    if (frame_back[g] < 1 || frame_back[g] > p->ring_n - 1)
      return fail(h, XK_EINVAL, "xk_trk_photo_spatial_add: frame_back outside 1...the ring's size - 1");
  }
  const size_t total = (size_t)off[G];
  if (total > 0 && (!pix_hist || !pix_cur || !o_hist || !o_cur)) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_add: null argument");
  if (s->state == XK_PSP_ESTIMATED) return XK_OK;                            // the map is installed: accumulation has stopped
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));                                // (the pinned staging is free)
  // one copy in: pixels | pixels | o_hist | o_cur | off | frame_back, packed for this call's total
  unsigned char *in = s->blk.h + up16(sizeof(XkPspState));
  size_t at = 0;
  XkPspAccArgs a = psp_acc_args(p, s, G);
  const auto put = [&](const void *src, size_t bytes) {
    const unsigned char *dev = s->d_in + at;
    if (bytes) memcpy(in + at, src, bytes);
    at += up16(bytes);
    return dev;
  };
  a.pix_hist = (const int *)put(pix_hist, 8 * total); a.pix_cur = (const int *)put(pix_cur, 8 * total);
  a.o_hist = (const double *)put(o_hist, 8 * total); a.o_cur = (const double *)put(o_cur, 8 * total);
  a.off = (const int *)put(off, sizeof(int) * (size_t)(G + 1)); a.frame_back = (const int *)put(frame_back, sizeof(int) * (size_t)G);
  HIPCHK(h, hipMemcpyAsync(s->d_in, in, at, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_photo_sp_accumulate, dim3(1), dim3(64), 0, h->stream, a);
  XKCHK(launched(h, "spatial accumulation launch"));
  return psp_fetch(h, s, "xk_trk_photo_spatial_add");
}

/* Where the accumulation stands */
extern "C" int xk_trk_photo_spatial_status(xk_trk *t, int *rows, int *covered, int *cells, int *ready, int *dropped, int *state) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_psp *s = psp_of(t, "xk_trk_photo_spatial_status");
  if (!s) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  XKCHK(psp_fetch(h, s, "xk_trk_photo_spatial_status"));
  const XkPspState *st = psp_host(s);
  if (st->rows < 0 || st->rows > s->max_rows || st->covered < 0 || st->covered > s->g.cells)
    return fail(h, XK_EDEVICE, "xk_trk_photo_spatial_status: state out of range");
  if (rows) *rows = st->rows;
  if (covered) *covered = st->covered;
  if (cells) *cells = s->g.cells;
  if (ready) *ready = st->ready;
  if (dropped) *dropped = st->dropped;
  if (state) *state = s->state;
  return XK_OK;
}

/* Rows first ... first+count-1, and the counts and coverage of every cell.  Straight copies */
extern "C" int xk_trk_photo_spatial_rows(xk_trk *t, int first, int count, int *sid_hist, int *sid_cur, double *b, int *counts,
                                         unsigned char *coverage) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_psp *s = psp_of(t, "xk_trk_photo_spatial_rows");
  if (!s) return XK_EINVAL;
  if (first < 0 || count < 0) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_rows: negative range");
  HIPCHK(h, hipSetDevice(h->device));
  XKCHK(psp_fetch(h, s, "xk_trk_photo_spatial_rows"));
  if (first + (long)count > psp_host(s)->rows) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_rows: range outside the accumulated rows");
  const size_t n = (size_t)count;
  if (sid_hist && n) HIPCHK(h, hipMemcpyAsync(sid_hist, s->sid_hist + first, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  if (sid_cur && n) HIPCHK(h, hipMemcpyAsync(sid_cur, s->sid_cur + first, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  if (b && n) HIPCHK(h, hipMemcpyAsync(b, s->b + first, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  if (counts) HIPCHK(h, hipMemcpyAsync(counts, s->count, sizeof(int) * (size_t)s->g.cells, hipMemcpyDeviceToHost, h->stream));
  if (coverage) HIPCHK(h, hipMemcpyAsync(coverage, s->coverage, (size_t)s->g.cells, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// One solve: the start, then batches of iterations with the done flag read through the pinned block after each.
static int psp_solve(xk_handle *h, xk_psp *s, XkPspPcgArgs a, int n, const XkPspSolve *rec_host) {
  hipLaunchKernelGGL(xk_photo_sp_pcg_init, dim3(1), dim3(XK_PSP_T), 0, h->stream, a);
  const int cap = a.cap > 0 ? a.cap : 2 * n, grid = (n + XK_PSP_MV_ROWS - 1) / XK_PSP_MV_ROWS;
  for (int queued = 0;;) {
    for (int i = 0; i < XK_PSP_BATCH && queued < cap; ++i, ++queued) {
      hipLaunchKernelGGL(xk_photo_sp_matvec, dim3(grid), dim3(64 * XK_PSP_MV_ROWS), 0, h->stream, a);
      hipLaunchKernelGGL(xk_photo_sp_step, dim3(1), dim3(XK_PSP_T), 0, h->stream, a);
    }
    XKCHK(launched(h, "spatial solve launch"));
    XKCHK(psp_fetch(h, s, "xk_trk_photo_spatial_estimate"));
    if (rec_host->done) return XK_OK;
    if (queued >= cap) return fail(h, XK_EDEVICE, "xk_trk_photo_spatial_estimate: the solve passed its cap without a done flag");
  }
}

/* IRPhotoCalib::EstimateSpatialParameters (irPhotoCalib.cpp:314-420) on the accumulated rows */
extern "C" int xk_trk_photo_spatial_estimate(xk_trk *t, int install, xk_photo_spatial_outcome *outcome) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_psp *s = psp_of(t, "xk_trk_photo_spatial_estimate");
  if (!s) return XK_EINVAL;
  xk_photo *p = t->klt->photo;
  if (!outcome) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_estimate: null argument");
  memset(outcome, 0, sizeof *outcome);
  HIPCHK(h, hipSetDevice(h->device));
  const XkPspState *st = psp_host(s);
  XKCHK(psp_fetch(h, s, "xk_trk_photo_spatial_estimate"));
  if (st->rows < 1) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_estimate: no row accumulated");
  s->staged_n = -1;
  // numbering, L and c, K
  XkPspNumArgs na{s->coverage, s->g.cells, s->n_max, s->var_of_cell, s->cell_of_var, s->st};
  hipLaunchKernelGGL(xk_photo_sp_number, dim3(1), dim3(XK_PSP_T), 0, h->stream, na);
  XkPspNormArgs ma{};
  ma.sid_hist = s->sid_hist; ma.sid_cur = s->sid_cur; ma.b = s->b; ma.var_of_cell = s->var_of_cell;
  ma.mult = (int *)s->K; ma.deg = s->deg; ma.L = s->L; ma.c = s->c; ma.diag = s->diag_l;
  ma.ld = s->ld; ma.n_max = s->n_max; ma.max_rows = s->max_rows; ma.st = s->st;
  hipLaunchKernelGGL(xk_photo_sp_clear, dim3(s->n_max), dim3(XK_PSP_T), 0, h->stream, ma);
  hipLaunchKernelGGL(xk_photo_sp_count, dim3((st->rows + XK_PSP_T - 1) / XK_PSP_T), dim3(XK_PSP_T), 0, h->stream, ma);
  hipLaunchKernelGGL(xk_photo_sp_normal, dim3((s->n_max + XK_PSP_T / 64 - 1) / (XK_PSP_T / 64)), dim3(XK_PSP_T), 0, h->stream, ma);
  XkPspGpArgs ga{};
  ga.cell_of_var = s->cell_of_var; ga.K = s->K; ga.diag = s->diag_k; ga.ld = s->ld; ga.n_max = s->n_max; ga.g = s->g;
  ga.sf2 = (double)s->gp_sf * (double)s->gp_sf; ga.sn2 = (double)s->gp_sn * (double)s->gp_sn;
  ga.inv2l2 = 1.0 / (2.0 * (double)s->gp_l * (double)s->gp_l);
  ga.alpha = s->alpha; ga.coarse = s->coarse; ga.ps = s->ps; ga.pitch = t->klt->slot[0].lv[0].pitch; ga.st = s->st;
  hipLaunchKernelGGL(xk_photo_sp_kernel, dim3(s->n_max), dim3(XK_PSP_T), 0, h->stream, ga);
  XKCHK(launched(h, "spatial normal-equation launch"));
  XKCHK(psp_fetch(h, s, "xk_trk_photo_spatial_estimate"));
  const int n = st->n;
  outcome->n = n;
  if (n > s->n_max) return fail(h, XK_ECAPACITY, "xk_trk_photo_spatial_estimate: more covered cells than n_max");
  if (n < 2) return fail(h, XK_EDEVICE, "xk_trk_photo_spatial_estimate: fewer than 2 unknowns");
  // the least squares, then the GP's weights on its solution
  XkPspPcgArgs pa{};
  pa.A = s->L; pa.rhs = s->c; pa.diag = s->diag_l; pa.x = s->x; pa.r = s->r; pa.p = s->p; pa.q = s->q; pa.partial = s->partial;
  pa.ld = s->ld; pa.n_max = s->n_max; pa.cap = h->opt_psp_cap; pa.s = &s->st->ls; pa.st = s->st;
  XKCHK(psp_solve(h, s, pa, n, &st->ls));
  pa.A = s->K; pa.rhs = s->x; pa.diag = s->diag_k; pa.x = s->alpha; pa.s = &s->st->gp; pa.after = &s->st->ls;
  XKCHK(psp_solve(h, s, pa, n, &st->gp));
  const bool ok = st->ls.converged && st->gp.converged;
  if (ok) {
    hipLaunchKernelGGL(xk_photo_sp_predict, dim3(s->g.cells), dim3(64), 0, h->stream, ga);
    XKCHK(launched(h, "spatial prediction launch"));
    if (install) HIPCHK(h, hipMemcpyAsync(p->PS, s->ps, sizeof(float) * (size_t)ga.pitch * s->g.h, hipMemcpyDeviceToDevice, h->stream));
    XKCHK(psp_fetch(h, s, "xk_trk_photo_spatial_estimate"));
  }
  outcome->converged = ok ? 1 : 0;
  outcome->ls_iterations = st->ls.it; outcome->gp_iterations = st->gp.it;
  outcome->ls_residual = st->ls.bb > 0.0 ? sqrt(st->ls.rr / st->ls.bb) : 0.0;
  outcome->gp_residual = st->gp.bb > 0.0 ? sqrt(st->gp.rr / st->gp.bb) : 0.0;
  s->staged_n = n;
  // not converging is an outcome, not an error: no map, and the accumulation goes on (irPhotoCalib.cpp:372-385)
  if (!ok) s->state = XK_PSP_FAILED;
  else if (install) s->state = XK_PSP_ESTIMATED;
  return XK_OK;
}

/* The last estimate's intermediates, for tests.  Straight copies; any pointer may be NULL */
extern "C" int xk_trk_photo_spatial_stage(xk_trk *t, int *var_of_cell, double *L, double *c, double *x, double *alpha, float *coarse, float *ps) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_psp *s = psp_of(t, "xk_trk_photo_spatial_stage");
  if (!s) return XK_EINVAL;
  if (s->staged_n < 0) return fail(h, XK_EINVAL, "xk_trk_photo_spatial_stage: no estimate since the setup or the last reset");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)s->staged_n, cells = (size_t)s->g.cells, pitch = (size_t)t->klt->slot[0].lv[0].pitch;
  if (var_of_cell) HIPCHK(h, hipMemcpyAsync(var_of_cell, s->var_of_cell, sizeof(int) * cells, hipMemcpyDeviceToHost, h->stream));
  if (L) HIPCHK(h, hipMemcpy2DAsync(L, 8 * n, s->L, 8 * (size_t)s->ld, 8 * n, n, hipMemcpyDeviceToHost, h->stream));
  if (c) HIPCHK(h, hipMemcpyAsync(c, s->c, 8 * n, hipMemcpyDeviceToHost, h->stream));
  if (x) HIPCHK(h, hipMemcpyAsync(x, s->x, 8 * n, hipMemcpyDeviceToHost, h->stream));
  if (alpha) HIPCHK(h, hipMemcpyAsync(alpha, s->alpha, 8 * n, hipMemcpyDeviceToHost, h->stream));
  if (coarse) HIPCHK(h, hipMemcpyAsync(coarse, s->coarse, sizeof(float) * cells, hipMemcpyDeviceToHost, h->stream));
  if (ps) HIPCHK(h, hipMemcpy2DAsync(ps, sizeof(float) * (size_t)s->g.w, s->ps, sizeof(float) * pitch, sizeof(float) * (size_t)s->g.w, (size_t)s->g.h,
                                    hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

/* Counts, coverage and rows back to empty, the state back to accumulating.  The PS plane keeps what it holds */
extern "C" int xk_trk_photo_spatial_reset(xk_trk *t) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_psp *s = psp_of(t, "xk_trk_photo_spatial_reset");
  if (!s) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  XKCHK(psp_queue_reset(h, s));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Normalisation and baseline check of the track manager's candidate tracks (track_manager.cpp:576-636), xk_tracks.hip.h
// ---------------------------------------------------------------------------
/* The capacities of one xk_trk_baseline call and its device and pinned blocks */
extern "C" int xk_trk_baseline_setup(xk_trk *t, int max_tracks, int max_obs) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  if (max_tracks < 1 || max_tracks > (1 << 20)) return fail(h, XK_EINVAL, "xk_trk_baseline_setup: max_tracks outside 1...2^20");
  if (max_obs < 1 || max_obs > (1 << 26)) return fail(h, XK_EINVAL, "xk_trk_baseline_setup: max_obs outside 1...2^26");
  HIPCHK(h, hipSetDevice(h->device));
  xk_bl *b = (xk_bl *)calloc(1, sizeof(xk_bl));
  if (!b) return XK_ENOMEM;
  b->max_tracks = max_tracks; b->max_obs = max_obs;
  size_t off = 0;
  const auto piece = [&off](size_t bytes) { const size_t at = off; off += up16(bytes); return at; };
  b->o_quat = piece(sizeof(double) * 4 * XK_TRACKS_MAX_QUATS);
  b->o_trk_off = piece(sizeof(int) * ((size_t)max_tracks + 1));
  b->o_norm_off = piece(sizeof(int) * ((size_t)max_tracks + 1));
  b->o_drop = piece((size_t)max_tracks);
  b->o_obs = piece(sizeof(double) * 2 * (size_t)max_obs);
  b->o_delta = piece(sizeof(double) * 2 * (size_t)max_tracks);
  b->o_flag = piece((size_t)max_tracks);
  b->o_norm = piece(sizeof(double) * 2 * (size_t)max_obs);
  const int rc = blk_alloc(h, b->blk, off, off, "xk_trk_baseline_setup");
  return setup_install(h, rc, "xk_trk_baseline_setup", t->bl, b);
}

/* Camera::normalize(track, list size) and TrackManager::checkBaseline of K tracks against one attitude list */
extern "C" int xk_trk_baseline(xk_trk *t, const int *trk_off, const double *obs_xy, const unsigned char *drop_last, int K, const double *C_q_G,
                               int n_quats, double min_baseline_x_n, double min_baseline_y_n, int *norm_off, double *norm_xy,
                               double *delta_xy, unsigned char *flag) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  const char *who = "xk_trk_baseline";
  xk_bl *b = t->bl;
  if (!b) return fail_at(h, XK_EINVAL, who, "before xk_trk_baseline_setup");
  if (K < 0 || !trk_off || !norm_off || (K > 0 && (!obs_xy || !drop_last || !C_q_G || !norm_xy || !delta_xy || !flag)))
    return fail_at(h, XK_EINVAL, who, "null argument or negative K");
  if (K > b->max_tracks) return fail_at(h, XK_EINVAL, who, "more tracks than max_tracks");
  if (n_quats < 2 || n_quats > XK_TRACKS_MAX_QUATS) return fail_at(h, XK_EINVAL, who, "n_quats outside 2...64");
  if (trk_off[0] < 0) return fail_at(h, XK_EINVAL, who, "trk_off is not monotone");
  int *h_norm_off = (int *)(b->blk.h + b->o_norm_off);          // built here, in the pinned block: it goes up with the rest
  h_norm_off[0] = 0;
  for (int k = 0; k < K; ++k) {
    const long long len = (long long)trk_off[k + 1] - trk_off[k];
    if (len < 0) return fail_at(h, XK_EINVAL, who, "trk_off is not monotone");
    if (trk_off[k + 1] > b->max_obs) return fail_at(h, XK_EINVAL, who, "more observations than max_obs");
    if (len < 2) return fail_at(h, XK_EINVAL, who, "a track of fewer than 2 observations");
    if (drop_last[k] > 1) return fail_at(h, XK_EINVAL, who, "drop_last is 0 or 1");
    const int nq = n_quats - (int)drop_last[k];
    if (nq < 2) return fail_at(h, XK_EINVAL, who, "an attitude list of fewer than 2 entries");   // (so the cropped length is >= 2 too)
    h_norm_off[k + 1] = h_norm_off[k] + (int)std::min<long long>(len, nq);
  }
  memcpy(norm_off, h_norm_off, sizeof(int) * ((size_t)K + 1));
  if (K == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n_obs = (size_t)trk_off[K], n_norm = (size_t)h_norm_off[K];
  memcpy(b->blk.h + b->o_quat, C_q_G, sizeof(double) * 4 * (size_t)n_quats);
  memcpy(b->blk.h + b->o_trk_off, trk_off, sizeof(int) * ((size_t)K + 1));
  memcpy(b->blk.h + b->o_drop, drop_last, (size_t)K);
  memcpy(b->blk.h + b->o_obs, obs_xy, sizeof(double) * 2 * n_obs);
  XkTracksArgs a{};
  a.quat = (const double *)(b->blk.d + b->o_quat); a.trk_off = (const int *)(b->blk.d + b->o_trk_off);
  a.norm_off = (const int *)(b->blk.d + b->o_norm_off); a.drop_last = b->blk.d + b->o_drop; a.obs_xy = (const double *)(b->blk.d + b->o_obs);
  a.K = K; a.n_quats = n_quats;
  a.fx = t->fx; a.fy = t->fy; a.cx = t->cx; a.cy = t->cy;
  a.min_x = min_baseline_x_n; a.min_y = min_baseline_y_n;
  a.norm_xy = (double *)(b->blk.d + b->o_norm); a.delta_xy = (double *)(b->blk.d + b->o_delta); a.flag = b->blk.d + b->o_flag;
  // one copy in, one launch, one copy out, one wait
  HIPCHK(h, hipMemcpyAsync(b->blk.d, b->blk.h, b->o_obs + sizeof(double) * 2 * n_obs, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_tracks_baseline, dim3((K + XK_TRACKS_WAVES - 1) / XK_TRACKS_WAVES), dim3(64 * XK_TRACKS_WAVES), 0, h->stream, a);
  XKCHK(launched(h, "baseline launch"));
  HIPCHK(h, hipMemcpyAsync(b->blk.h + b->o_delta, b->blk.d + b->o_delta, b->o_norm - b->o_delta + sizeof(double) * 2 * n_norm,
                           hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(norm_xy, b->blk.h + b->o_norm, sizeof(double) * 2 * n_norm);
  memcpy(delta_xy, b->blk.h + b->o_delta, sizeof(double) * 2 * (size_t)K);
  memcpy(flag, b->blk.h + b->o_flag, (size_t)K);
  return XK_OK;
}

// ---------------------------------------------------------------------------
// One frame of Tracker::track (tracker.cpp:134-306) on a feature list that stays on the device, xk_frame.hip.h
// ---------------------------------------------------------------------------
/* The parameters of Tracker::track as Tracker and its TiledImage hold them (tracker.h:234-261, tiled_image.cpp:98-105) and the resident list */
extern "C" int xk_trk_frame_setup(xk_trk *t, int n_feat_min, int n_tiles_h, int n_tiles_w, int max_feat_per_tile, double threshold_px,
                                  int n_hyp) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  if (!k) return fail(h, XK_EINVAL, "xk_trk_frame_setup: before xk_trk_klt_setup");
  const xk_det *d = k->det;
  const xk_orb *o = k->orb;
  if (!d) return fail(h, XK_EINVAL, "xk_trk_frame_setup: before xk_trk_detect_setup");
  if (n_feat_min < 0) return fail(h, XK_EINVAL, "xk_trk_frame_setup: n_feat_min < 0");
  if (n_tiles_h < 1 || n_tiles_w < 1 || (long long)n_tiles_h * n_tiles_w > XK_FRAME_MAX_TILES)
    return fail(h, XK_EINVAL, "xk_trk_frame_setup: tile counts outside 1...4096 tiles");
  if (max_feat_per_tile < 0) return fail(h, XK_EINVAL, "xk_trk_frame_setup: max_feat_per_tile < 0");
  if (!(threshold_px >= 0.0) || !std::isfinite(threshold_px)) return fail(h, XK_EINVAL, "xk_trk_frame_setup: threshold_px < 0");
  if (n_hyp < 1 || n_hyp > XK_FUND_MAX_HYP) return fail(h, XK_EINVAL, "xk_trk_frame_setup: n_hyp outside 1...4096");
  if (o && d->margin < o->edge)   // (a feature the description's filter dropped would have no descriptor to carry: FeatureTracker::detect throws there)
    return fail(h, XK_EINVAL, "xk_trk_frame_setup: the detection's margin is below the description's edge");
  HIPCHK(h, hipSetDevice(h->device));
  xk_frm *f = (xk_frm *)calloc(1, sizeof(xk_frm));
  if (!f) return XK_ENOMEM;
  f->n_feat_min = n_feat_min; f->tiles_h = n_tiles_h; f->tiles_w = n_tiles_w; f->max_per_tile = max_feat_per_tile;
  f->threshold_px = threshold_px; f->n_hyp = n_hyp;
  f->det = d; f->orb = o; f->n_res = -1; f->last_m = -1;
  const size_t M = (size_t)t->max_matches;
  f->cap_det = det_cap(t, d);
  f->cap_new = o ? std::min(f->cap_det, o->max_desc) : f->cap_det;
  const size_t N = (size_t)f->cap_new;
  const size_t klt_bytes = up16(klt_res_bytes(t->max_matches)), det_bytes = up16(det_res_bytes(t->max_matches));
  const size_t orb_bytes = o ? up16(xk_orb_res_bytes(N)) : 0, fund_bytes = up16(trk_res_total(t->max_matches));
  const size_t out_bytes = up16(xk_frame_out_bytes(M, o != nullptr)), desc_bytes = o ? up16(32 * M) : 0;
  const size_t d_bytes = up16(sizeof(int) * XK_FC_N) + up16(16 * M) + up16(8 * M) + up16(4 * M) + desc_bytes       // counts, resident list
                         + 2 * up16(4 * M) + 2 * up16(16 * M) + desc_bytes + up16(8 * N)                             // pair lists, new points
                         + 2 * klt_bytes + det_bytes + orb_bytes + fund_bytes + out_bytes;
  int rc = blk_alloc(h, f->blk, d_bytes, out_bytes, "xk_trk_frame_setup");
  if (rc == XK_OK && hipFuncSetAttribute((const void *)xk_fast_select, hipFuncAttributeMaxDynamicSharedMemorySize, XK_FAST_LDS_MAX) != hipSuccess)
    rc = fail(h, XK_ENOMEM, "xk_trk_frame_setup: allocation failed");
  if (rc == XK_OK) {
    XkFrameArgs &a = f->a;
    unsigned char *b = f->blk.d;
    size_t off = 0;
    a.c = carve<int>(b, off, sizeof(int) * XK_FC_N);
    a.res_dist = carve<double>(b, off, 16 * M);
    a.res_pts = carve<float>(b, off, 8 * M);
    a.res_score = carve<int>(b, off, 4 * M);
    a.res_desc = o ? carve<unsigned char>(b, off, 32 * M) : nullptr;
    a.l_score = carve<int>(b, off, 4 * M);
    a.l_origin = carve<int>(b, off, 4 * M);
    a.l_tiles = carve<int>(b, off, 16 * M);
    a.tmp_tiles = carve<int>(b, off, 16 * M);
    a.l_desc = o ? carve<unsigned char>(b, off, 32 * M) : nullptr;
    a.pts_new = carve<float>(b, off, 8 * N);
    f->klt_res[0] = carve<unsigned char>(b, off, klt_bytes);
    f->klt_res[1] = carve<unsigned char>(b, off, klt_bytes);
    a.det_res = carve<int>(b, off, det_bytes);
    f->orb_res = o ? carve<int>(b, off, orb_bytes) : nullptr;
    f->fund_res = carve<unsigned char>(b, off, fund_bytes);
    a.out = carve<unsigned char>(b, off, out_bytes);
    a.orb_res = f->orb_res;
    a.und = t->und;                                                 // (the outlier removal's scratch is the stage entries': every call fills it anew)
    a.n_feat_min = n_feat_min; a.tiles_h = n_tiles_h; a.tiles_w = n_tiles_w; a.max_per_tile = max_feat_per_tile;
    a.height = (double)k->height;
    a.tile_h = (double)k->height / n_tiles_h; a.tile_w = (double)k->width / n_tiles_w;        // tiled_image.cpp:104-105
    a.cap_new = f->cap_new; a.max_candidates = d->max_candidates; a.max_matches = t->max_matches; a.max_desc = o ? o->max_desc : 0;
  }
  return setup_install(h, rc, "xk_trk_frame_setup", k->frm, f);
}

/* The next frame is a first frame; the images stay */
extern "C" int xk_trk_frame_reset(xk_trk *t) {
  if (!t) return XK_EINVAL;
  xk_frm *f = sub_of(t, &xk_klt::frm, "xk_trk_frame_reset", "xk_trk_frame_setup");
  if (!f) return XK_EINVAL;
  f->n_res = -1; f->last_m = -1;
  return XK_OK;
}

/* The resident list as the device holds it.  Straight copies */
extern "C" int xk_trk_frame_features(xk_trk *t, double *dist_xy, int *score, unsigned char *desc, int *n) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_frm *f = sub_of(t, &xk_klt::frm, "xk_trk_frame_features", "xk_trk_frame_setup");
  if (!f) return XK_EINVAL;
  if (!n) return fail(h, XK_EINVAL, "xk_trk_frame_features: null count");
  const size_t r = (size_t)std::max(f->n_res, 0);
  *n = (int)r;
  if (r == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (dist_xy) HIPCHK(h, hipMemcpyAsync(dist_xy, f->a.res_dist, sizeof(double) * 2 * r, hipMemcpyDeviceToHost, h->stream));
  if (score) HIPCHK(h, hipMemcpyAsync(score, f->a.res_score, sizeof(int) * r, hipMemcpyDeviceToHost, h->stream));
  if (desc && f->a.res_desc) HIPCHK(h, hipMemcpyAsync(desc, f->a.res_desc, 32 * r, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

static const char *frame_status_text(int status) {
  switch (status) {
    case XK_FRAME_ECAND: return "more candidates than max_candidates";
    case XK_FRAME_EACCEPTED: return "more features accepted than max_matches";
    case XK_FRAME_EDESC: return "more keypoints than max_desc";
    case XK_FRAME_ETOTAL: return "old plus new features exceed max_matches";
  }
  return "status out of range";
}

// ---------------------------------------------------------------------------
// One frame of Tracker::track of a PHOTOMETRIC_CALI build (calibrateImage between the push and the tracking, tracker.cpp:186-190),
// xk_frame.hip.h with the intensities, xk_photo.hip.h fed from the resident list
// ---------------------------------------------------------------------------
/* n_hyp_photo caps the gain RANSAC of a frame; threshold_photo is fast_detection_delta_photo_ (tracker.cpp:848), < 0: no switch */
extern "C" int xk_trk_photo_frame_setup(xk_trk *t, int n_hyp_photo, int threshold_photo) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_frm *f = sub_of(t, &xk_klt::frm, "xk_trk_photo_frame_setup", "xk_trk_frame_setup");
  if (!f) return XK_EINVAL;
  xk_photo *p = sub_of(t, &xk_klt::photo, "xk_trk_photo_frame_setup", "xk_trk_photo_setup");
  if (!p) return XK_EINVAL;
  if (n_hyp_photo < 1 || n_hyp_photo > p->max_hyp) return fail(h, XK_EINVAL, "xk_trk_photo_frame_setup: n_hyp_photo outside 1...max_hyp");
  if (threshold_photo == 0 || threshold_photo > 254) return fail(h, XK_EINVAL, "xk_trk_photo_frame_setup: threshold_photo outside 1...254 (< 0: no switch)");
  HIPCHK(h, hipSetDevice(h->device));
  xk_pfrm *pf = (xk_pfrm *)calloc(1, sizeof(xk_pfrm));
  if (!pf) return XK_ENOMEM;
  pf->n_hyp = n_hyp_photo; pf->threshold = threshold_photo < 0 ? -1 : threshold_photo; pf->photo = p;
  const size_t M = (size_t)round_up(t->max_matches, 4), N = (size_t)round_up(f->cap_new, 4);
  const size_t out_bytes = up16(xk_frame_photo_out_bytes((size_t)t->max_matches, f->orb != nullptr));
  const size_t d_bytes = 4 * 8 * M + 2 * 8 * N + 8 * M + 8 * N + 2 * 4 * M + out_bytes;
  const int rc = blk_alloc(h, pf->blk, d_bytes, out_bytes, "xk_trk_photo_frame_setup");
  if (rc == XK_OK) {
    unsigned char *b = pf->blk.d;
    size_t off = 0;
    pf->res_int = carve<double>(b, off, 8 * M); pf->l_iprev = carve<double>(b, off, 8 * M); pf->l_icur = carve<double>(b, off, 8 * M);
    pf->val1 = carve<double>(b, off, 8 * M); pf->val_new = carve<double>(b, off, 8 * N); pf->val2 = carve<double>(b, off, 8 * N);
    pf->ixy1 = carve<int>(b, off, 8 * M); pf->ixy2 = carve<int>(b, off, 8 * N);
    pf->sum = carve<int>(b, off, 4 * M); pf->count = carve<int>(b, off, 4 * M);
    pf->out = carve<unsigned char>(b, off, out_bytes);
  }
  return setup_install(h, rc, "xk_trk_photo_frame_setup", f->pf, pf);
}

// The frame setup with its photometric part, both made over the setups still in place; or nullptr after fail(XK_EINVAL).
static xk_frm *photo_frame_of(xk_trk *t, const char *who) {
  xk_frm *f = sub_of(t, &xk_klt::frm, who, "xk_trk_frame_setup");
  if (!f) return nullptr;
  if (!f->pf || !t->klt->photo || f->pf->photo != t->klt->photo) {
    fail_at(t->h, XK_EINVAL, who, "before xk_trk_photo_frame_setup");
    return nullptr;
  }
  return f;
}

/* The resident intensities as the device holds them.  A straight copy */
extern "C" int xk_trk_photo_frame_intensities(xk_trk *t, double *intensity, int *n) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  xk_frm *f = photo_frame_of(t, "xk_trk_photo_frame_intensities");
  if (!f) return XK_EINVAL;
  if (!n) return fail(h, XK_EINVAL, "xk_trk_photo_frame_intensities: null count");
  const size_t r = (size_t)std::max(f->n_res, 0);
  *n = (int)r;
  if (r == 0 || !intensity) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(intensity, f->pf->res_int, sizeof(double) * r, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// Tracker::computeIntensity of the points at xy (their count on the device, at most n_bound) on level 0 of plane P, queued: values to `value`.
static void photo_frame_queue_intensity(xk_handle *h, const xk_photo *p, const xk_pfrm *pf, const XkKltPyr &P, const int *xy, const int *n_dev,
                                        int n_bound, double *value) {
  XkPhotoIntArgs a = photo_int_args(p, P.lv[0], n_bound);
  a.xy = xy; a.n_dev = n_dev; a.value = value; a.sum = pf->sum; a.count = pf->count;
  hipLaunchKernelGGL(xk_photo_intensity, dim3((n_bound + XK_PHOTO_WAVES - 1) / XK_PHOTO_WAVES), dim3(64 * XK_PHOTO_WAVES), 0, h->stream, a);
}

// The kept current points of a tracking truncated to pixels, and their intensities on level 0 of plane P, queued.
static void photo_frame_queue_kept_intensity(xk_handle *h, const xk_photo *p, const xk_pfrm *pf, const XkKltPyr &P, const XkKeptPairs &kept,
                                             int n_bound, int *ixy, double *value) {
  XkFrameTruncArgs ta{};
  ta.xy = kept.kept_cur; ta.n_dev = kept.res; ta.n = n_bound; ta.ixy = ixy;
  hipLaunchKernelGGL(xk_frame_trunc, dim3((n_bound + 255) / 256), dim3(256), 0, h->stream, ta);
  photo_frame_queue_intensity(h, p, pf, P, ixy, kept.res, n_bound, value);
}

// ---------------------------------------------------------------------------
// The body of both frames.  The kernels of xk_frame.hip.h treat the plain frame as the photometric one with res_int == NULL; so does the host
// ---------------------------------------------------------------------------
// What xk_trk_photo_frame has beyond xk_trk_frame: the seed of the gain RANSAC and its own outputs.  Its setups are k->photo and f->pf.
struct frame_photo {
  unsigned long seed;
  xk_trk_photo_frame_out *out;
};

// featureDetection of a frame on the working plane of slot s and its gate, queued; then, of the accepted features, the intensities on that
// plane (pf: the photometric frame, tracker.cpp:461) and the description.  Old features and pred as det_queue's.
static int frame_queue_detect(xk_trk *t, const xk_frm *f, const XkFrameArgs &a, const xk_pfrm *pf, int s, const double *old_xy, int n_old,
                              const int *n_old_dev, const int *pred) {
  xk_handle *h = t->h;
  XKCHK(det_queue(t, s, a.det_res, old_xy, n_old, n_old_dev, pred, pf ? pf->threshold : -1));
  hipLaunchKernelGGL(xk_frame_gate, dim3(1), dim3(256), 0, h->stream, a);
  if (pf) photo_frame_queue_intensity(h, t->klt->photo, pf, t->klt->slot[s], a.det_res + 4, a.c + XK_FC_NEW, f->cap_new, pf->val_new);
  return f->orb ? orb_queue(t, s, a.det_res + 4, f->orb_res, f->cap_new, a.c + XK_FC_NEW, pred) : XK_OK;
}

// featureTracking on the WORKING planes of the n points at pts (with n_dev, the device's count of at most n), queued: the resident list
// (which = 0) or the re-detection's features (1), the result block goes to f->klt_res[which].  The photometric frame adds the kept current
// features' intensities on the RAW current plane at the truncated pixel (tracker.cpp:666).
static int frame_queue_track(xk_trk *t, const xk_frm *f, const xk_pfrm *pf, int which, const float *pts, int n, const int *n_dev) {
  xk_klt *k = t->klt;
  XkKltArgs ka;
  XKCHK(klt_queue_track(t->h, k, pf ? 0 : k->sel, pf ? &k->photo->st->done : nullptr, k->slot[k->cur ^ 1], k->slot[k->cur], pts, f->klt_res[which],
                        n, ka, n_dev));
  if (pf) photo_frame_queue_kept_intensity(t->h, k->photo, pf, k->photo->raw[k->cur], ka.kept, n, which ? pf->ixy2 : pf->ixy1,
                                           which ? pf->val2 : pf->val1);
  return XK_OK;
}

// Tracker::track (tracker.cpp:134-306), pyramid level 0, for entry `who`: everything queued on the handle's stream, one copy out, one wait.
// ph: the photometric frame, whose result block and pinned mirror are the xk_pfrm's; without it they are the frame setup's.
static int frame_run(xk_trk *t, xk_frm *f, const char *who, const unsigned char *img, int stride, unsigned long seed, xk_trk_frame_out *out,
                     const frame_photo *ph) {
  xk_handle *h = t->h;
  xk_klt *k = t->klt;
  xk_photo *p = ph ? k->photo : nullptr;
  xk_pfrm *pf = ph ? f->pf : nullptr;
  xk_trk_photo_frame_out *pout = ph ? ph->out : nullptr;
  if (!img || stride < k->width) return fail_at(h, XK_EINVAL, who, "null image or stride below the width");
  if (!out || !out->prev_xy || !out->cur_xy || !out->prev_dist_xy || !out->cur_dist_xy || !out->score || !out->origin || !out->tiles ||
      (f->orb && !out->desc) || (ph && (!pout->prev_intensity || !pout->cur_intensity)))
    return fail_at(h, XK_EINVAL, who, "null output");
  out->n_tracked = out->n_left = out->redetected = out->n_candidates = out->n_accepted = out->n_new_tracked = out->n_matches = 0;
  out->winner = -1;
  if (ph) {
    pout->n_cal_kept = pout->estimated = pout->support = 0;
    pout->done = p->done;
    pout->a_rel = 1.0; pout->b_rel = 0.0;
    memset(pout->frame_ab, 0, sizeof pout->frame_ab);
  }
  HIPCHK(h, hipSetDevice(h->device));
  const bool first = f->n_res < 0, desc = f->orb != nullptr;
  const int M = t->max_matches, R = first ? 0 : f->n_res;
  const int n_hyp_photo = ph ? std::max(1, std::min(R, pf->n_hyp)) : 0;
  f->n_res = -1;                                                    // (whatever fails below: the next frame is a first frame)
  f->last_m = -1;
  t->lmeds_hyp = 0;                                                 // (and this one has run no LMedS yet)
  XKCHK(trk_push(t, img, stride));
  XkFrameArgs a = f->a;
  a.first = first ? 1 : 0;
  a.n_res = R;
  a.B = first ? 1 : std::min(M, R + f->cap_det);
  const size_t B = (size_t)a.B;
  a.l_prev = t->dist; a.l_cur = t->dist + 2 * B;
  if (ph) {
    a.out = pf->out;
    a.res_int = pf->res_int; a.l_iprev = pf->l_iprev; a.l_icur = pf->l_icur;
    a.val1 = pf->val1; a.val_new = pf->val_new; a.val2 = pf->val2;
    a.photo_st = p->st;
  }
  int *c = a.c;
  unsigned char *r = ph ? pf->blk.h : f->blk.h;
  const int *head = (const int *)r;
  size_t out_bytes = sizeof(int) * XK_FC_N;
  if (first) {
    XKCHK(frame_queue_detect(t, f, a, pf, k->cur, nullptr, 0, nullptr, nullptr));
    hipLaunchKernelGGL(xk_frame_first, dim3((f->cap_new + 255) / 256), dim3(256), 0, h->stream, a);
  } else {
    // 2. calibrateImage as xk_trk_photo_calibrate queues it, from the resident points and intensities; with fewer than 4 features
    // (tracker.cpp:763) only the correction, which corrects iff an earlier frame estimated
    if (ph) {
      memset(p->n_hyp, 0, sizeof p->n_hyp);
      XkKeptPairs cal;
      if (R >= 4) {
        XKCHK(photo_queue_calibrate(t, a.res_pts, pf->res_int, R, n_hyp_photo, ph->seed, cal));
        a.cal_kept = cal.res;
      }
      XKCHK(photo_queue_correct(h, k, k->cur, 1));
    }
    a.kept1 = klt_kept_at(f->klt_res[0], R);
    a.kept2 = klt_kept_at(f->klt_res[1], f->cap_new);
    XkFundArgs fa = trk_args(t, f->fund_res, a.B, c + XK_FC_TOTAL);
    a.kept3 = fa.kept;
    t->n_hyp = 0;                                                   // (the scratch no longer holds the last xk_trk_filter_matches)
    trk_note_call(t, t->method, 0, f->fund_res, a.B);
    // 3. the resident list from the previous image to the current one, its post-filter; 4. the overflow pass (both intensities move with their pair)
    if (R > 0) XKCHK(frame_queue_track(t, f, pf, 0, a.res_pts, R, nullptr));
    hipLaunchKernelGGL(xk_frame_overflow, dim3(1), dim3(256), sizeof(int) * (size_t)f->tiles_h * f->tiles_w, h->stream, a);
    // 5. the re-detection on the PREVIOUS image, queued on every frame and predicated on the flag the overflow pass left.  (With
    // n_feat_min = 0 the flag is never set: nothing is queued, and xk_frame_concat finds the zero count the overflow pass wrote.)
    if (f->n_feat_min > 0) {
      XKCHK(frame_queue_detect(t, f, a, pf, k->cur ^ 1, a.l_prev, R, c + XK_FC_LEFT, c + XK_FC_REDETECT));
      XKCHK(frame_queue_track(t, f, pf, 1, a.pts_new, f->cap_new, c + XK_FC_NEW));
    }
    hipLaunchKernelGGL(xk_frame_concat, dim3(1), dim3(256), 0, h->stream, a);
    // 6. the outlier removal; 7. the result block (the calibration's outcome in its head) and the new resident list
    XKCHK(trk_queue_ransac(h, fa, t->method, true, f->threshold_px, f->n_hyp, seed));
    hipLaunchKernelGGL(xk_frame_pack, dim3((a.B + 255) / 256), dim3(256), 0, h->stream, a);
    out_bytes = ph ? xk_frame_photo_out_bytes(B, desc) : xk_frame_out_bytes(B, desc);
  }
  XKCHK(launched(h, first ? "first frame launch" : "frame launch"));
  HIPCHK(h, hipMemcpyAsync(r, a.out, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));                       // the frame's one wait
  const int status = head[XK_FC_STATUS], m = head[XK_FC_MATCHES];
  bool ok = m >= 0 && m <= a.B && status >= 0 && status <= XK_FRAME_ETOTAL;
  for (int j = 0; j <= XK_FC_TOTAL; ++j) ok = ok && head[j] >= 0 && (j == XK_FC_CAND || j == XK_FC_ACCEPTED || head[j] <= M);
  if (ph) ok = ok && head[XK_FC_RING_N] >= 1 && head[XK_FC_RING_N] <= XK_PHOTO_RING && head[XK_FC_CAL_KEPT] >= 0 && head[XK_FC_CAL_KEPT] <= R;
  if (!ok) return fail_at(h, XK_EDEVICE, who, "counts out of range");
  out->n_tracked = head[XK_FC_TRACKED]; out->n_left = head[XK_FC_LEFT]; out->redetected = head[XK_FC_REDETECT];
  out->n_candidates = head[XK_FC_CAND]; out->n_accepted = head[XK_FC_ACCEPTED]; out->n_new_tracked = head[XK_FC_NEW_TRACKED];
  out->winner = head[XK_FC_WINNER];
  if (ph) {                                                         // the calibration's outcome, and the host's mirrors of the photometric state
    p->ring_n = head[XK_FC_RING_N]; p->done = head[XK_FC_DONE];
    if (head[XK_FC_CAL_KEPT] > 4) p->n_hyp[0] = n_hyp_photo;
    pout->n_cal_kept = head[XK_FC_CAL_KEPT]; pout->estimated = head[XK_FC_ESTIMATED]; pout->done = head[XK_FC_DONE];
    pout->support = head[XK_FC_SUPPORT];
    if (!first) {
      const double *calv = (const double *)(r + xk_frame_out_cal(B, desc));
      pout->a_rel = calv[0]; pout->b_rel = calv[1];
      memcpy(pout->frame_ab, calv + 2, sizeof pout->frame_ab);
    }
  }
  if (status != 0) return fail_at(h, XK_ECAPACITY, who, frame_status_text(status));
  if (first) {
    f->n_res = head[XK_FC_NEW];
    f->last_m = 0;
    return XK_OK;
  }
  trk_note_call(t, t->method, f->n_hyp, f->fund_res, a.B);
  out->n_matches = m;
  memcpy(out->prev_xy, r + xk_frame_out_xy(B, 0), sizeof(double) * 2 * (size_t)m);
  memcpy(out->cur_xy, r + xk_frame_out_xy(B, 1), sizeof(double) * 2 * (size_t)m);
  memcpy(out->prev_dist_xy, r + xk_frame_out_xy(B, 2), sizeof(double) * 2 * (size_t)m);
  memcpy(out->cur_dist_xy, r + xk_frame_out_xy(B, 3), sizeof(double) * 2 * (size_t)m);
  memcpy(out->score, r + xk_frame_out_score(B), sizeof(int) * (size_t)m);
  memcpy(out->origin, r + xk_frame_out_origin(B), sizeof(int) * (size_t)m);
  memcpy(out->tiles, r + xk_frame_out_tiles(B), sizeof(int) * 4 * (size_t)m);
  if (desc) memcpy(out->desc, r + xk_frame_out_desc(B), 32 * (size_t)m);
  if (ph) {
    memcpy(pout->prev_intensity, r + xk_frame_out_int(B, desc, 0), sizeof(double) * (size_t)m);
    memcpy(pout->cur_intensity, r + xk_frame_out_int(B, desc, 1), sizeof(double) * (size_t)m);
  }
  f->n_res = m;
  f->last_m = m; f->last_B = a.B; f->last_out = a.out;
  return XK_OK;
}

/* Tracker::track of a build without PHOTOMETRIC_CALI */
extern "C" int xk_trk_frame(xk_trk *t, const unsigned char *img, int stride, unsigned long seed, xk_trk_frame_out *out) {
  if (!t) return XK_EINVAL;
  xk_frm *f = sub_of(t, &xk_klt::frm, "xk_trk_frame", "xk_trk_frame_setup");
  if (!f) return XK_EINVAL;
  if (t->klt->photo) return fail(t->h, XK_EINVAL, "xk_trk_frame: a photometric setup is in place (the photometric frame is xk_trk_photo_frame)");
  return frame_run(t, f, "xk_trk_frame", img, stride, seed, out, nullptr);
}

/* Tracker::track of a build with PHOTOMETRIC_CALI.  xk_trk_photo_frame_out begins with the fields of xk_trk_frame_out: the body fills those
 * through a copy of that part, and the outputs this frame adds in place */
extern "C" int xk_trk_photo_frame(xk_trk *t, const unsigned char *img, int stride, unsigned long seed, unsigned long seed_photo,
                                  xk_trk_photo_frame_out *out) {
  static_assert(offsetof(xk_trk_photo_frame_out, prev_intensity) == sizeof(xk_trk_frame_out), "xk_trk_photo_frame_out begins with xk_trk_frame_out");
  if (!t) return XK_EINVAL;
  xk_frm *f = photo_frame_of(t, "xk_trk_photo_frame");
  if (!f) return XK_EINVAL;
  const frame_photo ph{seed_photo, out};
  xk_trk_frame_out o;
  if (out) memcpy(&o, out, sizeof o);
  const int rc = frame_run(t, f, "xk_trk_photo_frame", img, stride, seed, out ? &o : nullptr, &ph);
  if (out) memcpy(out, &o, sizeof o);
  return rc;
}

// ---------------------------------------------------------------------------
// TrackManager::manageTracks on tracks that stay on the device (track_manager.cpp:115-436), xk_track_store.hip.h
// ---------------------------------------------------------------------------
// The result block of one call, laid out by the host's bounds: head | lost [lost] | claimed [n] | entry starts, lengths [entries] each |
// entry ids [entries] | normalised coordinates [obs][2].
struct xk_ts_layout {
  size_t o_lost, o_claimed, o_start, o_len, o_id, o_xy, bytes;
};

static xk_ts_layout ts_layout(size_t lost, size_t n, size_t entries, size_t obs) {
  xk_ts_layout L{};
  size_t off = up16(sizeof(int) * XK_TSR_N);
  const auto piece = [&off](size_t bytes) { const size_t at = off; off += up16(bytes); return at; };
  L.o_lost = piece(sizeof(int) * lost); L.o_claimed = piece(sizeof(int) * n);
  L.o_start = piece(sizeof(int) * entries); L.o_len = piece(sizeof(int) * entries); L.o_id = piece(sizeof(long long) * entries);
  L.o_xy = piece(sizeof(double) * 2 * obs);
  L.bytes = off;
  return L;
}

/* The store, its scratch, the staging of a call's inputs and the result block with its pinned mirror */
extern "C" int xk_trk_tracks_setup(xk_trk *t, int max_tracks, int n_tiles_h, int n_tiles_w, int width, int height, double min_baseline_x_n,
                                   double min_baseline_y_n, int multi_uav) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  const char *who = "xk_trk_tracks_setup";
  if (max_tracks < 1 || max_tracks > (1 << 20)) return fail_at(h, XK_EINVAL, who, "max_tracks outside 1...2^20");
  if (n_tiles_h < 1 || n_tiles_w < 1 || (long long)n_tiles_h * n_tiles_w > XK_TS_MAX_TILES) return fail_at(h, XK_EINVAL, who, "tile counts outside 1...4096 tiles");
  if (width < 1 || height < 1) return fail_at(h, XK_EINVAL, who, "image size below 1 x 1");
  if (min_baseline_x_n != min_baseline_x_n || min_baseline_y_n != min_baseline_y_n) return fail_at(h, XK_EINVAL, who, "a baseline threshold is not a number");
  if (multi_uav < 0 || multi_uav > 1) return fail_at(h, XK_EINVAL, who, "multi_uav is 0 or 1");
  HIPCHK(h, hipSetDevice(h->device));
  xk_ts *s = (xk_ts *)calloc(1, sizeof(xk_ts));
  if (!s) return XK_ENOMEM;
  s->max_tracks = max_tracks; s->max_n = t->max_matches;
  const size_t T = (size_t)max_tracks, M = (size_t)t->max_matches, R = XK_TS_RING;
  s->in_bytes = up16(sizeof(double) * 4 * XK_TRACKS_MAX_QUATS) + up16(sizeof(long long) * T) + 4 * up16(sizeof(double) * 2 * M) + up16(sizeof(int) * M);
  s->out_bytes = ts_layout(T, M, T + M, (T + M) * R).bytes;
  s->gather_bytes = up16(8 * T) + up16(4 * T) + up16(32 * R * T) + up16(4 * R * T) + up16(8 * R * T);
  const size_t store = up16(32 * R * T) + up16(4 * R * T) + up16(8 * R * T) + up16(4 * T) + up16(8 * T) + 4 * up16(4 * T) + 2 * 16;
  const size_t scratch = up16(sizeof(int) * XK_TSC_N) + up16(16 * M) + 5 * up16(4 * M) + up16(16 * T) + 18 * up16(4 * T) + up16(4 * (T + 1)) * 2 +
                         2 * up16(T) + up16(16 * T) + up16(16 * R * T);
  const int rc = blk_alloc(h, s->blk, store + scratch + s->in_bytes + s->out_bytes + s->gather_bytes, s->in_bytes + s->out_bytes, who);
  if (rc == XK_OK) {
    XkTsArgs &a = s->a;
    unsigned char *b = s->blk.d;
    size_t off = 0;
    a.obs = carve<double>(b, off, 32 * R * T); a.score = carve<int>(b, off, 4 * R * T); a.tile = carve<int>(b, off, 8 * R * T);
    a.len = carve<int>(b, off, 4 * T); a.id = carve<long long>(b, off, 8 * T);
    a.slam = carve<int>(b, off, 4 * T); a.newl = carve<int>(b, off, 4 * T); a.opp = carve<int>(b, off, 4 * T); a.free_ = carve<int>(b, off, 4 * T);
    a.hdr = carve<int>(b, off, sizeof(int) * XK_TSH_N); a.next_id = carve<long long>(b, off, 8);
    a.c = carve<int>(b, off, sizeof(int) * XK_TSC_N);
    a.m_tile = carve<int>(b, off, 16 * M);
    a.m_bin = carve<int>(b, off, 4 * M); a.m_owner = carve<int>(b, off, 4 * M); a.rm = carve<int>(b, off, 4 * M); a.mo = carve<int>(b, off, 4 * M);
    a.newk = carve<int>(b, off, 4 * M);
    a.last_xy = carve<double>(b, off, 16 * T);
    int **per_track[] = {&a.pm, &a.kp, &a.lost_slot, &a.o_owner, &a.o_claimed, &a.comb, &a.cbin, &a.corig, &a.calive, &a.opp_tmp, &a.dead, &a.sorted,
                         &a.lens, &a.act, &a.cand_of, &a.cand_slot, &a.l_msckf, &a.l_short};
    for (int **p : per_track) *p = carve<int>(b, off, 4 * T);
    a.trk_off = carve<int>(b, off, 4 * (T + 1)); a.norm_off = carve<int>(b, off, 4 * (T + 1));
    a.drop = carve<unsigned char>(b, off, T); a.flag = carve<unsigned char>(b, off, T);
    a.delta = carve<double>(b, off, 16 * T);
    a.b_obs = carve<double>(b, off, 16 * R * T);
    s->d_in = carve<unsigned char>(b, off, s->in_bytes);
    s->d_out = carve<unsigned char>(b, off, s->out_bytes);
    s->d_gather = carve<unsigned char>(b, off, s->gather_bytes);
    a.max_tracks = max_tracks; a.multi_uav = multi_uav;
    a.tiles_h = n_tiles_h; a.tiles_w = n_tiles_w;
    a.height = (double)height; a.tile_h = (double)height / n_tiles_h; a.tile_w = (double)width / n_tiles_w;   // tiled_image.cpp:104-105
    a.fx = t->fx; a.fy = t->fy; a.cx = t->cx; a.cy = t->cy; a.min_x = min_baseline_x_n; a.min_y = min_baseline_y_n;
    hipLaunchKernelGGL(xk_ts_clear, dim3((max_tracks + 255) / 256), dim3(256), 0, h->stream, a, 1);
  }
  return setup_install(h, rc == XK_OK ? launched(h, "track store setup launch") : rc, who, t->ts, s);
}

static xk_ts *ts_of(xk_trk *t, const char *who) {
  if (!t->ts) fail_at(t->h, XK_EINVAL, who, "before xk_trk_tracks_setup");
  return t->ts;
}

// Both manage entries.  host: the match columns on the host (copied up with the attitudes), or dev: the same columns on the device.
struct ts_matches {
  const double *prev_xy, *cur_xy, *prev_dist_xy, *cur_dist_xy;
  const int *score;
};

static int ts_manage(xk_trk *t, xk_ts *s, const char *who, const ts_matches *host, const ts_matches *dev, int n, const double *C_q_G, int n_quats,
                     int n_poses_max, int n_slam_features_max, int min_track_length, long long *opp_ids, int *n_opp_ids, xk_trk_tracks_out *out) {
  xk_handle *h = t->h;
  const int n_ids = n_opp_ids ? *n_opp_ids : 0;
  if (n < 0 || n > s->max_n) return fail_at(h, XK_EINVAL, who, "n outside 0...max_matches");
  if (host && n > 0 && (!host->prev_xy || !host->cur_xy || !host->prev_dist_xy || !host->cur_dist_xy || !host->score))
    return fail_at(h, XK_EINVAL, who, "null match column");
  if (!C_q_G || n_quats < 3 || n_quats > XK_TRACKS_MAX_QUATS) return fail_at(h, XK_EINVAL, who, "3...64 camera attitudes");
  if (n_poses_max < 3) return fail_at(h, XK_EINVAL, who, "n_poses_max < 3");
  if (n_slam_features_max < 0) return fail_at(h, XK_EINVAL, who, "n_slam_features_max < 0");
  if (min_track_length < 1 || min_track_length > n_poses_max) return fail_at(h, XK_EINVAL, who, "min_track_length outside 1...n_poses_max");
  if (n_ids < 0 || n_ids > s->max_tracks || (n_ids > 0 && !opp_ids)) return fail_at(h, XK_EINVAL, who, "opp_ids: null, or their number outside 0...max_tracks");
  if (s->a.multi_uav && !n_opp_ids) return fail_at(h, XK_EINVAL, who, "multi_uav without an id list");
  const size_t P = (size_t)s->n_slam + s->n_new, O = (size_t)s->n_opp;
  const size_t entries = O + n + P, obs = (O + n) * (size_t)n_quats + P * (size_t)std::min(n_poses_max, XK_TS_RING);
  if (!out || !out->claimed || !out->lost_slam_idxs || !out->ids || !out->off || !out->xy) return fail_at(h, XK_EINVAL, who, "null output");
  if ((size_t)std::max(out->cap_lost, 0) < P || (size_t)std::max(out->cap_entries, 0) < entries || (size_t)std::max(out->cap_obs, 0) < obs)
    return fail_at(h, XK_EINVAL, who, "an output capacity is below the call's bound");
  HIPCHK(h, hipSetDevice(h->device));
  const xk_ts_layout L = ts_layout(P, (size_t)n, entries, obs);
  XkTsArgs a = s->a;
  a.n = n; a.n_quats = n_quats; a.n_poses_max = n_poses_max; a.n_slam_max = n_slam_features_max; a.min_track_length = min_track_length;
  a.n_opp_ids = n_ids;
  // the inputs: attitudes | ids | the match columns (host-fed), one copy
  unsigned char *hi = s->blk.h;
  size_t off = 0;
  const auto put = [&](const void *src, size_t bytes) {
    const size_t at = off;
    if (bytes) memcpy(hi + at, src, bytes);
    off += up16(bytes);
    return s->d_in + at;
  };
  a.quat = (const double *)put(C_q_G, sizeof(double) * 4 * (size_t)n_quats);
  a.opp_ids = (const long long *)put(opp_ids, sizeof(long long) * (size_t)n_ids);
  if (host) {
    a.m_prev = (const double *)put(host->prev_xy, 16 * (size_t)n); a.m_cur = (const double *)put(host->cur_xy, 16 * (size_t)n);
    a.m_dprev = (const double *)put(host->prev_dist_xy, 16 * (size_t)n); a.m_dcur = (const double *)put(host->cur_dist_xy, 16 * (size_t)n);
    a.m_score = (const int *)put(host->score, 4 * (size_t)n);
  } else {
    a.m_prev = dev->prev_xy; a.m_cur = dev->cur_xy; a.m_dprev = dev->prev_dist_xy; a.m_dcur = dev->cur_dist_xy; a.m_score = dev->score;
  }
  unsigned char *d = s->d_out, *r = s->blk.h + s->in_bytes;
  a.head = (int *)d; a.lost = (int *)(d + L.o_lost); a.claimed = (int *)(d + L.o_claimed); a.e_start = (int *)(d + L.o_start);
  a.e_len = (int *)(d + L.o_len); a.e_id = (long long *)(d + L.o_id); a.norm_xy = (double *)(d + L.o_xy);
  // one copy in, four launches, one copy out, one wait
  HIPCHK(h, hipMemcpyAsync(s->d_in, hi, off, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_ts_associate, dim3(1), dim3(XK_TS_THREADS), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ts_candidates, dim3(1), dim3(XK_TS_THREADS), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ts_baseline, dim3((unsigned)((O + n + XK_TRACKS_WAVES) / XK_TRACKS_WAVES)), dim3(64 * XK_TRACKS_WAVES), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ts_walk, dim3(1), dim3(64), 0, h->stream, a);
  XKCHK(launched(h, "track manager launch"));
  HIPCHK(h, hipMemcpyAsync(r, d, L.bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int *head = (const int *)r;
  const int status = head[XK_TSR_STATUS];
  out->status = status;
  out->n_persistent = head[XK_TSR_N_SLAM]; out->n_new_persistent = head[XK_TSR_N_NEW]; out->n_opportunistic = head[XK_TSR_N_OPP];
  out->n_lost = head[XK_TSR_N_LOST]; out->n_claimed = head[XK_TSR_N_CLAIMED]; out->n_candidates = head[XK_TSR_N_CAND];
  out->n_candidate_obs = head[XK_TSR_N_CAND_OBS];
  out->next_id = (long long)(((unsigned long long)(unsigned int)head[XK_TSR_NEXT_ID_HI] << 32) | (unsigned int)head[XK_TSR_NEXT_ID_LO]);
  for (int l = 0; l < 5; ++l) out->n_list[l] = 0;
  if (status == XK_TS_EOUTSIDE) return fail_at(h, XK_EINVAL, who, "a match outside the tile grid");
  if (status == XK_TS_ECAPACITY) return fail_at(h, XK_ECAPACITY, who, "the frame may have more candidate or live tracks than max_tracks");
  if (status == XK_TS_EBOOKKEEPING) return fail_at(h, XK_EDEVICE, who, "tile bookkeeping out of step");
  size_t n_entries = 0;
  bool ok = status == 0 && head[XK_TSR_N_LOST] >= 0 && (size_t)head[XK_TSR_N_LOST] <= P && head[XK_TSR_N_NORM] >= 0 && head[XK_TSR_N_PER_OBS] >= 0 &&
            (size_t)head[XK_TSR_N_NORM] + (size_t)head[XK_TSR_N_PER_OBS] <= obs && head[XK_TSR_N_SLAM] >= 0 && head[XK_TSR_N_NEW] >= 0 &&
            head[XK_TSR_N_OPP] >= 0 && (long long)head[XK_TSR_N_SLAM] + head[XK_TSR_N_NEW] + head[XK_TSR_N_OPP] <= s->max_tracks;
  for (int l = 0; l < 5 && ok; ++l) {
    ok = head[XK_TSR_LIST0 + l] >= 0 && (size_t)head[XK_TSR_LIST0 + l] <= entries;
    n_entries += (size_t)std::max(head[XK_TSR_LIST0 + l], 0);
  }
  if (!ok || n_entries > entries) return fail_at(h, XK_EDEVICE, who, "counts out of range");
  s->n_slam = head[XK_TSR_N_SLAM]; s->n_new = head[XK_TSR_N_NEW]; s->n_opp = head[XK_TSR_N_OPP];
  for (int l = 0; l < 5; ++l) out->n_list[l] = head[XK_TSR_LIST0 + l];
  memcpy(out->lost_slam_idxs, r + L.o_lost, sizeof(int) * (size_t)out->n_lost);
  const int *claimed = (const int *)(r + L.o_claimed);
  for (int i = 0; i < n; ++i) out->claimed[i] = claimed[i] ? 1 : 0;
  // the lists behind one another as one CSR: a list's coordinates are gathered in its order (a candidate's lie where the batch put them)
  const int *e_start = (const int *)(r + L.o_start), *e_len = (const int *)(r + L.o_len);
  const double *xy = (const double *)(r + L.o_xy);
  memcpy(out->ids, r + L.o_id, sizeof(long long) * n_entries);
  out->off[0] = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    if (e_len[e] < 0 || e_start[e] < 0 || (size_t)e_start[e] + (size_t)e_len[e] > obs || (size_t)out->off[e] + (size_t)e_len[e] > obs)
      return fail_at(h, XK_EDEVICE, who, "counts out of range");
    memcpy(out->xy + 2 * (size_t)out->off[e], xy + 2 * (size_t)e_start[e], sizeof(double) * 2 * (size_t)e_len[e]);
    out->off[e + 1] = out->off[e] + e_len[e];
  }
  if (n_opp_ids) *n_opp_ids = 0;                                    // the caller's list is consumed (track_manager.cpp:355)
  return XK_OK;
}

/* manageTracks of a match list from the host */
extern "C" int xk_trk_tracks_manage(xk_trk *t, const double *prev_xy, const double *cur_xy, const double *prev_dist_xy, const double *cur_dist_xy,
                                    const int *score, int n, const double *C_q_G, int n_quats, int n_poses_max, int n_slam_features_max,
                                    int min_track_length, long long *opp_ids, int *n_opp_ids, xk_trk_tracks_out *out) {
  if (!t) return XK_EINVAL;
  xk_ts *s = ts_of(t, "xk_trk_tracks_manage");
  if (!s) return XK_EINVAL;
  const ts_matches m{prev_xy, cur_xy, prev_dist_xy, cur_dist_xy, score};
  return ts_manage(t, s, "xk_trk_tracks_manage", &m, nullptr, n, C_q_G, n_quats, n_poses_max, n_slam_features_max, min_track_length, opp_ids,
                   n_opp_ids, out);
}

/* manageTracks of the matches the last frame left on the device */
extern "C" int xk_trk_tracks_manage_frame(xk_trk *t, const double *C_q_G, int n_quats, int n_poses_max, int n_slam_features_max,
                                          int min_track_length, long long *opp_ids, int *n_opp_ids, xk_trk_tracks_out *out) {
  if (!t) return XK_EINVAL;
  const char *who = "xk_trk_tracks_manage_frame";
  xk_ts *s = ts_of(t, who);
  if (!s) return XK_EINVAL;
  xk_frm *f = sub_of(t, &xk_klt::frm, who, "xk_trk_frame_setup");
  if (!f) return XK_EINVAL;
  if (f->last_m < 0) return fail_at(t->h, XK_EINVAL, who, "no frame result on the device (before a frame, after xk_trk_frame_reset or a frame's error)");
  const size_t B = (size_t)f->last_B;
  const unsigned char *o = f->last_out;
  ts_matches m{};
  if (f->last_m > 0) {
    m.prev_xy = (const double *)(o + xk_frame_out_xy(B, 0)); m.cur_xy = (const double *)(o + xk_frame_out_xy(B, 1));
    m.prev_dist_xy = (const double *)(o + xk_frame_out_xy(B, 2)); m.cur_dist_xy = (const double *)(o + xk_frame_out_xy(B, 3));
    m.score = (const int *)(o + xk_frame_out_score(B));
  }
  return ts_manage(t, s, who, nullptr, &m, f->last_m, C_q_G, n_quats, n_poses_max, n_slam_features_max, min_track_length, opp_ids, n_opp_ids, out);
}

/* One of the store's own lists */
extern "C" int xk_trk_tracks_lists(xk_trk *t, int which, long long *ids, int *lengths, double *obs, int *score, int *tiles, int *n) {
  if (!t) return XK_EINVAL;
  xk_handle *h = t->h;
  const char *who = "xk_trk_tracks_lists";
  xk_ts *s = ts_of(t, who);
  if (!s) return XK_EINVAL;
  if (which < 0 || which > 2) return fail_at(h, XK_EINVAL, who, "which is 0, 1 or 2");
  if (!n) return fail_at(h, XK_EINVAL, who, "null count");
  const size_t N = (size_t)(which == 0 ? s->n_slam : which == 1 ? s->n_new : s->n_opp), T = (size_t)s->max_tracks, R = XK_TS_RING;
  *n = (int)N;
  if (N == 0 || (!ids && !lengths && !obs && !score && !tiles)) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  XkTsListOut o{};
  size_t off = 0;
  o.which = which; o.n = (int)N;
  o.ids = carve<long long>(s->d_gather, off, 8 * T); o.lengths = carve<int>(s->d_gather, off, 4 * T); o.obs = carve<double>(s->d_gather, off, 32 * R * T);
  o.score = carve<int>(s->d_gather, off, 4 * R * T); o.tiles = carve<int>(s->d_gather, off, 8 * R * T);
  hipLaunchKernelGGL(xk_ts_gather, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, h->stream, s->a, o);
  XKCHK(launched(h, "track list launch"));
  if (ids) HIPCHK(h, hipMemcpyAsync(ids, o.ids, 8 * N, hipMemcpyDeviceToHost, h->stream));
  if (lengths) HIPCHK(h, hipMemcpyAsync(lengths, o.lengths, 4 * N, hipMemcpyDeviceToHost, h->stream));
  if (obs) HIPCHK(h, hipMemcpyAsync(obs, o.obs, 32 * R * N, hipMemcpyDeviceToHost, h->stream));
  if (score) HIPCHK(h, hipMemcpyAsync(score, o.score, 4 * R * N, hipMemcpyDeviceToHost, h->stream));
  if (tiles) HIPCHK(h, hipMemcpyAsync(tiles, o.tiles, 8 * R * N, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// erase of ascending list positions, the highest XK_TS_REMOVE_MAX first: a launch does not move what lies below its positions
static int ts_remove(xk_trk *t, xk_ts *s, int which, const unsigned int *idxs, int n) {
  HIPCHK(t->h, hipSetDevice(t->h->device));
  for (int end = n; end > 0; end -= XK_TS_REMOVE_MAX) {
    XkTsRemove r{};
    const int first = std::max(end - XK_TS_REMOVE_MAX, 0);
    r.which = which; r.n = end - first;
    for (int j = 0; j < r.n; ++j) r.idx[j] = (int)idxs[first + j];
    hipLaunchKernelGGL(xk_ts_remove, dim3(1), dim3(64), 0, t->h->stream, s->a, r);
  }
  XKCHK(launched(t->h, "track removal launch"));
  (which == 0 ? s->n_slam : s->n_new) -= n;
  return XK_OK;
}

/* removePersistentTracksAtIndex */
extern "C" int xk_trk_tracks_remove_persistent(xk_trk *t, unsigned int idx) {
  if (!t) return XK_EINVAL;
  xk_ts *s = ts_of(t, "xk_trk_tracks_remove_persistent");
  if (!s) return XK_EINVAL;
  if (idx >= (unsigned int)s->n_slam) return fail_at(t->h, XK_EINVAL, "xk_trk_tracks_remove_persistent", "no such track");
  return ts_remove(t, s, 0, &idx, 1);
}

/* removeNewPersistentTracksAtIndexes */
extern "C" int xk_trk_tracks_remove_new_persistent(xk_trk *t, const unsigned int *idxs, int n) {
  if (!t) return XK_EINVAL;
  const char *who = "xk_trk_tracks_remove_new_persistent";
  xk_ts *s = ts_of(t, who);
  if (!s) return XK_EINVAL;
  if (n < 0 || (n > 0 && !idxs)) return fail_at(t->h, XK_EINVAL, who, "null indices or negative n");
  for (int i = 0; i < n; ++i) {
    if (idxs[i] >= (unsigned int)s->n_new) return fail_at(t->h, XK_EINVAL, who, "no such track");
    if (i > 0 && idxs[i] <= idxs[i - 1]) return fail_at(t->h, XK_EINVAL, who, "indices not in increasing order");
  }
  return n == 0 ? XK_OK : ts_remove(t, s, 1, idxs, n);
}

/* TrackManager::clear: the lists empty, the id counter as it was */
extern "C" int xk_trk_tracks_clear(xk_trk *t) {
  if (!t) return XK_EINVAL;
  xk_ts *s = ts_of(t, "xk_trk_tracks_clear");
  if (!s) return XK_EINVAL;
  HIPCHK(t->h, hipSetDevice(t->h->device));
  hipLaunchKernelGGL(xk_ts_clear, dim3((s->max_tracks + 255) / 256), dim3(256), 0, t->h->stream, s->a, 0);
  XKCHK(launched(t->h, "track store clear launch"));
  s->n_slam = s->n_new = s->n_opp = 0;
  return XK_OK;
}
