// xk_handle.hip.h -- the engine's handle and the small helpers every part of xk_api.hip's translation unit uses on it.  Included by xk_api.hip only.
#pragma once

#define XK_STAGE_SLOTS 8
#define XK_PDBG_WORDS 65536     // debug stamps of the single launch (lab build)

// What the last compression left behind: the schedule that served the update and the few facts its readers need (compressed_spec,
// eval_status, xk_caqr_status, xk_bench_staged, the callers that skip launch_update after a fused launch).  launch_compress writes it
// once, whole, when a schedule has queued its work.  (Which tail geometry a multi-launch update took is not kept: nothing reads it
// once the launches are queued.)
enum XkSchedule {
  XK_SCHED_NONE = 0,       // nothing compressed yet (or launch_build has taken d_R2 back from rows that went to the update as built)
  XK_SCHED_EMPTY,          // no measurement row at all: [T_H | z] = 0
  XK_SCHED_SLAM_ROWS,      // d_R2 = the SLAM features' rows as built, no track in the stack (split_plan 2)
  XK_SCHED_SMALL_STACK,    // d_R2 = a small stack as built (split_plan 3)
  XK_SCHED_SINGLE,         // one launch of xk_caqr_pipe: the whole stack into d_R
  XK_SCHED_SINGLE_SPLIT,   // ... the split form: the tracks' rows into d_R2, the SLAM rows as built behind them (split_plan 1)
  XK_SCHED_MULTI,          // the multi-launch CAQR into d_R
  XK_SCHED_MULTI_TAIL,     // ... its last columns in one or two launches of xk_caqr_pipe<XkPipeTail / XkPipeTail4>
};
struct XkOutcome {
  XkSchedule schedule;
  bool fused;              // the single launch also carried the Kalman update (posterior in d_Pout, correction written)
  bool narrow2;            // the last SINGLE launch ran in the 152-tile geometry; the other schedules carry it over (the give-up word
                           // eval_status reads after them can only be that launch's)
  int leaves, launches;    // tiles of the first level / launches behind the first one (xk_bench_staged: n_leaf, n_levels)
};
// the system in d_R2 that compressed_spec follows, in split_plan's numbering (0: d_R)
static inline int outcome_R2_mode(const XkOutcome &o) { return o.schedule == XK_SCHED_SINGLE_SPLIT ? 1 : o.schedule == XK_SCHED_SLAM_ROWS ? 2 : o.schedule == XK_SCHED_SMALL_STACK ? 3 : 0; }
// launch_build: d_R2 belongs to the update being built.  The record stops naming a system there; the schedule it reports is otherwise kept.
static inline void outcome_release_R2(XkOutcome &o) {
  if (o.schedule == XK_SCHED_SINGLE_SPLIT) o.schedule = XK_SCHED_SINGLE;
  else if (o.schedule == XK_SCHED_SLAM_ROWS || o.schedule == XK_SCHED_SMALL_STACK) o.schedule = XK_SCHED_NONE;
}
static inline bool outcome_single(const XkOutcome &o) { return o.schedule == XK_SCHED_SINGLE || o.schedule == XK_SCHED_SINGLE_SPLIT; }
// the schedule word of xk_caqr_status (include/xk.h): 4 nothing compressed, 3 multi-launch + tail, 2 single launch, 0 multi-launch or none yet
static inline int outcome_status(const XkOutcome &o) {
  return o.schedule == XK_SCHED_NONE || o.schedule == XK_SCHED_MULTI ? 0 : outcome_single(o) ? 2 : o.schedule == XK_SCHED_MULTI_TAIL ? 3 : 4;
}

// How far the update of the staged inputs has got, and what of it is still owed to xk_apply_update.  One record: the entries of
// xk_update_api.hip.h raise the stage as they queue work, and pending_drop (below) takes the whole record back to "staged" -- the stage
// is lowered nowhere else.  Plain data: the handle is calloc'ed.
enum XkUpdateStage {
  XK_UPD_STAGED = 0,       // inputs staged, or none yet: no rows of theirs on the device
  XK_UPD_ROWS,             // launch_build has queued the rows
  XK_UPD_ROWS_DEFERRED,    // ... and xk_build_compress_async has left the compression to xk_apply_update, where the Kalman role can ride
                           // along on the covariance the applyCI entries in between have left (MULTI_UAV order)
  XK_UPD_COMPRESSED,       // launch_compress has queued [T_H | z]: xk_handle::last says where it is
  XK_UPD_QUEUED,           // ... and the Kalman update is queued behind it (xk_build_compress_update[_pass]_async): xk_apply_update only waits
};
struct XkPending {
  XkUpdateStage stage;
  bool unread;             // the status words of the queued launches have yet to be read: whoever reads them (settle_async,
                           // xk_apply_update) owns the retry if the single-launch CAQR gave up
  // XK_UPD_QUEUED: what the queued pass was asked for -- xk_apply_update must ask the same -- and its completion marker
  int cov_update;
  bool ct_zero;            // correction_total NULL or all zero
  double *ct;              // ... else its n doubles (allocated by xk_create)
  unsigned long long seq;  // the marker xk_apply_update waits for (0: for the stream)
};

struct xk_handle {
  int device;
  hipStream_t stream;
  hipStream_t copy_stream;   // gate flags travel to the host beside the QR kernels, not between them
  hipEvent_t ev_flags, ev_flags_done;
  hipEvent_t ev[16];
  // capacities
  int N, Mmax, Kmax, n, na, C1, C1P, DB, ntiles_max;
  // staged problem
  int n_poses, K, M;
  size_t obs_cap;
  double *d_q, *d_p, *d_obs, *d_feat, *d_zlast;
  int *d_trk_off, *d_anchor;
  double *d_chi_s;        // [Mmax] chi-square threshold of each staged SLAM feature (xk_stage_slam)
  int chi_far_dof[8];     // the thresholds past the table that xk_stage_slam computed last (a feature's dof grows by 2 per frame)
  double chi_far_val[8];
  int chi_far_next;
  double *d_P, *d_Pout;
  double *d_Psnap;        // xk_snapshot_P (slot of the caller)
  double *d_Psnap2;       // ... slot of the filter loop (x::Ekf saves the prior of an update the IMU thread may lap)
  double *d_fq;           // f_d, q_d of xk_cov_propagate
  double *d_chi95;
  double *d_A;
  double *d_Hc;            // factor records of the MSCKF tracks (xk_feature.hip.h: XkFeatArgs::Hc), hc_stride doubles each, 64-row slots only
  int hc_stride;
  int opt_hlite;           // 1 (default): the per-feature kernel leaves factor records when the single launch is expected to run
  int opt_psp_cap;         // lab: > 0 caps the iterations of both solves of xk_trk_photo_spatial_estimate (0: 2 n, the statement's cap)
  int opt_gate_form;       // 1 (default): gate of tracks of <= 32 observations by generalised least squares (XkFeatArgs::gate_form); lab: 0 = the projected form everywhere
  bool rows_compact;       // the last build left records, not tiles, for slots [0, K)
  int *d_tile_rows;
  double *d_panel[2];   // CAQR: 16 x 16 panel blocks of the even (tiles, level 2, ..) / odd merge levels
  int *d_inl, *d_inl_s, *d_gn;
  double *d_gam, *d_gam_s, *d_gpf;
  double *d_R;
  // single-launch CAQR (xk_caqr_pipe.hip.h): cross-XCD exchange slabs, XCD-local strips and panel blocks,
  // two sets of sync words (a launch uses one and zeroes the other for its successor)
  double *d_x1;            // both sets of the cross-XCD slabs (X1 | X2 | X1P each)
  size_t xslab_doubles;    // ... doubles per set
  double *d_rs, *d_rpb;
  unsigned *d_xsync;
  int xsync_phase;
  int pipe_rows_nominal;   // rows the last single launch was queued for, every track counted as accepted
  // Geometry with two first-level groups per XCD (XkPipeNarrow2: 152 tiles): taken when the rows expected to pass the gates fit it.
  // The expectation is the acceptance ratio the last single launch reported (status word 2) applied to this update's nominal rows.
  int opt_split;           // 0 never, 1 adaptive (default); lab: 2 whenever the NOMINAL rows fit, 3 always
  double acc_ratio;        // accepted / nominal rows of the last single launch (0: none yet)
  int pipe_tag;            // tag of the last single launch's accepted-rows word (status word 2)
  int split_backoff;       // updates for which it stays off after it found more rows than it holds
  int overflow_rows;       // a single launch of that many nominal rows found more accepted rows than its tiles hold: not tried again at that size
  // SPLIT compression (round 6; systems with SLAM features whose update cannot ride inside the launch, n > 206: BASELINE config 2).
  // The rows of MSCKF tracks are zero in the features' columns (msckf_update.cpp:412-416) and the features' own rows are 2 M in number:
  // only the tracks' rows need compressing, and only in the 6 N pose columns (+ the residual) -- a system of <= 199 columns instead of
  // 6 N + 3 M + 1.  T = [R1 | 0 | z1 ; H_slam | res_slam] (6 N + 2 M rows, T^T T = H^T H and T^T z = H^T res exactly as for the R of
  // the whole stack) goes to d_R2; xk_qr_compress, which hands out the reference's upper-triangular T_H, keeps compressing everything.
  double *d_R2;         // [C1P][C1P] row-major: rows [0, 6 N) = R1 of the tracks' rows, rows [6 N, 6 N + 2 M) = the SLAM rows as built
  XkOutcome last;       // what the last launch_compress left (in d_R or d_R2: compressed_spec follows it)
  int plan;             // split_plan of the staged update, latched by launch_build: the rows were built for it (tiles or factor records), and
                        // launch_compress and compressed_spec take it -- an option changed in between does not split the two
  bool d_R2_dirty;      // a small stack (plan 3) left dense rows in d_R2: the next split compression clears rows [0, 6 N) before it writes R1
  bool want_full_T;     // xk_qr_compress is running: compress everything into d_R
  int opt_slam_split;
  int opt_pipe_min_rows;   // nominal rows from which the single launch is queued (1; lab: XK_PIPE_MIN_ROWS)
  // Tall systems (128-row slots: windows of 34..64 poses, BASELINE config 3): the multi-launch schedule factors the first panels,
  // ONE launch of xk_caqr_pipe<XkPipeTail> the last <= 96 columns with every row in registers (round 6)
  bool tail_capable;    // decided at xk_create: 128-row slots, 256 CUs, the kernel fits a CU
  bool tail_ok;         // armed (cleared when a tail launch gave up; re-armed like the fast path)
  int tail_backoff_len; // updates the tail stays off after it found more rows than it holds (reason 9): 64, doubling while that keeps happening
  int tail_clean, tail_backoff, opt_tail;   // opt_tail: 0 off, 1 (default) the plan that fits (192 columns in one or two launches, else 96 in one), 2 the 96-column launch only
  long long *d_pdbg;
  long long *feat_dbg;  // probe builds only: per-workgroup phase stamps of xk_msckf_feature
  bool attr_slaminit, attr_feat_batch;   // hipFuncSetAttribute done for this handle's device
  int n_cu;
  bool persist_ok;      // cleared when a launch gave up (workgroups not co-resident): the multi-launch schedule takes over
  bool fast_capable;    // decided at xk_create: 256 CUs, one 768-thread workgroup of the single-launch kernels fits a CU
  int fast_giveups, fast_reason;   // launches that gave up so far / why the last one did (xk_caqr_status)
  int clean_classic, rearm_after;  // multi-launch updates since the last give-up / how many of them re-arm the fast path
  // experiment switches and test hooks of the compression, read from the environment ONCE at xk_create (the per-update path
  // calls no getenv); xk_set_option changes them on a live handle (tests do)
  int opt_resident, opt_poison, opt_test_stall, opt_tall26;
  int opt_kalman;          // the Kalman update inside the single launch (xk_pipe_kalman) where the geometry allows it
  XkPending upd;           // the staged update: how far it has got, what xk_apply_update has to collect
  bool xsync_dirty;     // a pipelined launch gave up: its counters are mid-count, clear both sets before the next one
  double sigma_img;
  // update workspace
  int CM, LDA;
  double *d_Maug, *d_X, *d_corr, *d_ct, *d_tmpH, *d_tmpS, *d_tmpP, *d_rdiag, *d_tmpz;
  double *h_win;        // host copy of the staged window lists (7 doubles per pose), see flush_window
  bool win_pending;     // ... which have not reached d_q / d_p yet
  bool win_valid;       // h_win holds the lists of the window in use
  unsigned *d_done_cnt;  // workgroup counter of the completion marker
  unsigned long long done_seq, done_seen, flags_after_seq;   // completion markers (XK_SPIN_DONE): launched / seen / launched when the gate flags were queued
  int *d_status;        // status words; they live in PINNED HOST memory (h_out + n): kernels write them only on failure
  double *h_out;        // pinned host, device-visible: [n] correction of xk_apply_update + the status words
  // CI / payload
  double *d_payload;
  double *d_ci;  // scratch for the CI kernels
  double *d_ciws;          // workspace of the device-resident CI round (lazily allocated): eight regions of ci_track_ws (xk_ci_api.hip.h)
  // CI weight search (xk_ciw.hip.h): option "ci_weight_search"; d_ciw = [8 weights | 8 start | 2 info words | 8 M_i | 8 H_i P_i H_i^T]
  int opt_ci_search;
  double *d_ciw;
  double ci_last_w[8];     // what xk_ci_last_weights hands out: the weights of the last searched entry,
  int ci_last_k1, ci_last_iters;   // how many there were and the Newton steps they took
  // searched device round (xk_ciw_round.hip.h), allocated by the first searched round:
  // d_ciwr = per agent [Maug | X] (n x (n + 168) each), then the solver's operands and results: ciwr_layout (xk_ci_api.hip.h)
  double *d_ciwr;
  int ci_round_tracks;             // shared tracks of the last searched round (0 before the first one)
  double ci_round_w[8][8];         // what xk_ci_round_weights hands out
  int ci_round_k1[8], ci_round_iters[8];
  hipStream_t ci_stream[8];   // ... and its side streams: shared track j >= 1 runs its stages before the gate on ci_stream[j],
  hipEvent_t ci_fork, ci_join[8];   // next to track 0 on the engine's stream (forked and joined with events)
  XkFeatBatch *d_batch;    // per-agent descriptors of the batched feature launch, [8 tracks][8 agents]
  XkFeatBatch *h_batch;    // pinned staging of the same
  double *h_ci_w;          // pinned: what the round's kernels report to the host (the XK_CIP_* words of xk_ciw_round.hip.h)
  int *h_trk_off;          // host copy of the staged track offsets
  // MSCKF-SLAM tracks (features being initialised this frame)
  int anchor_max;          // largest staged SLAM anchor index (rechecked against the staged window at build time)
  int K2;
  bool ms_built;           // their column-space rows on the device belong to the staged tracks
  int *d_trk2_off, *h_trk2_off, *d_inl2, *d_gn2;
  double *d_obs2, *d_gpf2, *d_W2, *d_gam2, *d_H1, *d_H2, *d_r1, *d_feat2;
  int *d_csr_i;            // sparse congruence operand: row pointers then column indices
  double *d_csr_v;         //   and values
  size_t csr_cap;          //   capacity in non-zeros
  // pinned staging ring for inputs copied to the device WITHOUT a host synchronisation (window, tracks, sparse operands):
  // a slot is reused XK_STAGE_SLOTS calls later, by which time an update's final synchronisation has long passed
  char *h_stage[XK_STAGE_SLOTS];
  int stage_since_sync;    // slots handed out since the stream was last known to be idle (stage_slot)
  size_t stage_bytes;
  int stage_next;
  bool flags_direct;       // no SLAM rows in the last build: nothing was copied, the kernel wrote the cache
  bool flags_cached;       // h_flag_* hold the gate results of the last build (fetched with the update's status)
  int *h_flag_i;
  double *h_flag_d;
  char *trk_slot;          // xk_stage_tracks_begin .. _end: the staging slot being filled
  int trk_slot_K, trk_slot_nobs;
  // range-facet / sun-angle rows (xk_stage_range / xk_stage_sun_angle, xk_aux.hip.h).  Staged measurements wait in aux_in until the next
  // build, which consumes them (the reference uses a measurement once: timestamp = -1, vio_updater.cpp:380,402) and fixes the plan of that
  // update in aux_mask / naux: which rows, how many, and which variances they carry.  A replay of the same update (a retry after a single
  // launch gave up, xk_run_steps, xk_bench_staged) rebuilds them from the same staged measurement; a build with nothing staged has none.
  XkAuxIn aux_in;
  int aux_staged;          // 1 range, 2 sun: staged since the last build
  int aux_mask;            // ... the rows of the current update
  int naux;                // 0..3 rows appended to the system the update applies
  double *d_aux;           // [naux x (n + 1) rows | rdiag 3 | flags 2]
  double *d_Taug;          // the applied system with the rows appended: CM x (n + 1) row-major, then CM variances
  // host pinned staging
  double *h_pin;
  size_t h_pin_doubles;
  int *h_pin_i;
  char err[256];
};

// Back to "staged", whole: the stage, a deferred compression, a queued pass and what it was asked for, status words nobody has read.
// Everything that invalidates the rows or the compressed system calls this -- staging, a rewritten covariance (congruence, propagation,
// the device CI round), a give-up, a new build, the end of an update -- and nothing else lowers the stage.
static inline void pending_drop(xk_handle *h) {
  double *ct = h->upd.ct;
  memset(&h->upd, 0, sizeof(h->upd));
  h->upd.ct = ct;
}

static int fail(xk_handle *h, int code, const char *what, hipError_t e = hipSuccess) {
  if (h) {
    if (e != hipSuccess) snprintf(h->err, sizeof(h->err), "%s: %s", what, hipGetErrorString(e));
    else snprintf(h->err, sizeof(h->err), "%s", what);
  }
  return code;
}
#define HIPCHK(h, call)                                                   \
  do {                                                                    \
    hipError_t e_ = (call);                                               \
    if (e_ != hipSuccess) return fail((h), XK_EDEVICE, #call, e_);        \
  } while (0)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

template <typename T>
static hipError_t dalloc(T **p, size_t count) {
  return hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
}

// Experiment switches.  The RELEASE library (libxk.so) never looks at the environment: every switch has its default.  The LAB
// build (-DXK_LAB: x_multi_agent_amd/lab/libxk.so, include/xk_lab.h) reads them -- once each -- and carries the test hooks,
// the debug exports and the probe kernels the tests and tools/exp use.
#ifdef XK_LAB
static int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v ? atoi(v) : dflt;
}
#else
static inline int env_int(const char *, int dflt) { return dflt; }
#endif
