// xk_compress.hip.h -- host side of the measurement compression (vio_updater.cpp:487-512): which schedule serves the staged stack and the
// launches of each, the system they leave for the Kalman update (compressed_spec), the reading of the status words.  Included by
// xk_update_api.hip.h only (xk_api.hip's translation unit), behind launch_build; the two small kernels here keep their place among the
// __global__ functions of that translation unit.
#pragma once
#include <type_traits>

// The stack of an update that is NOT compressed (rows <= columns: vio_updater.cpp:487 compresses only `if (h.rows() > h.cols())`): slot t's rows
// -- the tile the per-feature kernel left -- go to rows [off_t, off_t + 2 L_t - 3) of T, off_t = 2 trk_off[t] - 3 t (every track counted in:
// the host queues the update before it knows the gates' verdicts); a rejected track's rows (tile_rows = 0) are zero rows, which the update
// ignores (a zero row of H with noise sigma^2 moves nothing).  One workgroup per slot.
__global__ __launch_bounds__(256) void xk_stack_rows(const double *A, const int *tile_rows, const int *trk_off, int DB, int C1P, int row0, double *T) {
  const int t = blockIdx.x;
  const int nr = 2 * (trk_off[t + 1] - trk_off[t]) - 3, off = row0 + 2 * trk_off[t] - 3 * t, valid = min(tile_rows[t], nr);
  const double *src = A + (size_t)t * DB * C1P;
  double *dst = T + (size_t)off * C1P;
  for (int e = threadIdx.x; e < nr * C1P; e += blockDim.x) dst[e] = (e / C1P < valid) ? src[e] : 0.0;
}

__global__ void xk_mark_done(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }

struct UpdateSpec {
  const double *T;   // c x kdim measurement matrix over state columns [col0, col0+kdim)
  long str, stc;
  int c, kdim, col0;
  const double *z;   // residual (device), stride sz
  long sz;
  const double *rdiag;  // device vector (c) or null -> rscalar
  double rscalar;
  const double *S;   // externally supplied innovation covariance (device, row stride ss, col stride 1)... or null
  long ssr, ssc;
  const double *Pin;  // n x n col-major
  double *Pout;       // n x n col-major (may equal neither Pin)
  const double *ct;   // device corr_total or null
  int cov_update;
  double *corr;       // where the correction goes: null -> h->d_corr (device); xk_apply_update passes pinned host memory
  unsigned long long *done_flag;   // optional completion marker (pinned host memory) written by the last launch ...
  unsigned long long done_seq;     // ... with this value
  int tri;           // T is upper trapezoidal (T[r][k] == 0 for k < r: the compressed R): the products skip the zero blocks
  int naux;          // range / sun rows of this update (d_aux) to append: launch_update applies [T ; rows] over all n columns
};

// ---------------------------------------------------------------------------
// switches, row counts and the predicates the schedules share
// ---------------------------------------------------------------------------
// Experiment switches of the compression (lab build: the environment, include/xk_lab.h; the release build: the defaults), read
// once, ALL of them by the first compression of the process (a variable set in the environment after that is not seen, whichever
// schedule would have been the first to look at it): the per-update path calls no getenv.
struct XkCompressEnv {
  int wt, arity1, chalf, overlap, skip_rejected, persist_dbg, lchalf, adapt, cus, m32;
};
static const XkCompressEnv &compress_env() {
  static const XkCompressEnv e = {env_int("XK_CAQR_WT", 0),       env_int("XK_CAQR_ARITY1", 0),        env_int("XK_CAQR_CHALF", 8),
                                  env_int("XK_CAQR_OVERLAP", 1),  env_int("XK_CAQR_SKIP_REJECTED", 1), env_int("XK_CAQR_PERSIST_DBG", 0),
                                  env_int("XK_CAQR_LCHALF", 0),   env_int("XK_CAQR_ADAPT", 1),         env_int("XK_CAQR_CUS", 256),
                                  env_int("XK_CAQR_M32", 1)};
  return e;
}

// Nominal rows of slot t (every track counted as accepted: the host queues before it knows the gates' verdicts) -- MSCKF tracks, then
// the tracks that become features, 2 L - 3 each, then the SLAM rows packed DB to a slot (vio_updater.cpp:406-422)
static int slot_rows_nominal(const xk_handle *h, int t) {
  if (t < h->K) return 2 * (h->h_trk_off[t + 1] - h->h_trk_off[t]) - 3;
  if (t < h->K + h->K2) return 2 * (h->h_trk2_off[t - h->K + 1] - h->h_trk2_off[t - h->K]) - 3;
  return std::min(h->DB, 2 * h->M - (t - h->K - h->K2) * h->DB);
}
// ... of the tracks' slots together: what the split form compresses, and what a stack has on top of its 2 M SLAM rows
static long split_rows_nominal(const xk_handle *h) {
  long r = 0;
  for (int t = 0; t < h->K + h->K2; ++t) r += slot_rows_nominal(h, t);
  return r;
}

// rows the tiles of the single launch hold, by the columns of the system it factors
static int pipe_rows_cap(int cols) { return cols <= XkPipeNarrow::COLS ? XkPipeNarrow::ROWS : XkPipeWide::ROWS; }
// Is the single launch queued for R nominal rows in `nslots` slots?  The launch compacts the stack itself (xk_pipe_rowplan: rows of
// rejected tracks cost nothing), so what its tiles must hold is the rows that PASS the gates -- which the host does not know when it
// queues.  It queues on the nominal count up to a quarter over the capacity; a launch that finds more accepted rows than its tiles
// hold gives up at once (reason 9) and the multi-launch schedule serves the update -- and the following ones of that size.
static bool pipe_queueable(const xk_handle *h, long R, int nslots, int rows_cap) {
  return R >= h->opt_pipe_min_rows && nslots <= XK_PIPE_SLOTS_MAX && R * 4 <= (long)rows_cap * 5 && (h->overflow_rows == 0 || R < h->overflow_rows);
}
// Can the Kalman update ride inside the single launch on this handle?  The narrow geometry of the WHOLE stack: the split form, whose
// system has 6 N + 1 columns instead of C1, exists only where n > 206 (split_plan), so C1 is the launch's column count here.
static bool kalman_rides(const xk_handle *h) { return h->opt_kalman && h->C1 <= XkPipeNarrow::COLS && h->n <= 206 && h->n_cu == 256; }

// Will the compression of the staged update take the split form?  Evaluated once per build (launch_build latches it in h->plan) for
// compressed_spec -- which callers evaluate BEFORE launch_compress -- and for launch_compress itself; a split system goes nowhere but
// into the single launch, so plan 1 asks pipe_queueable what compress_single will ask.
static int split_plan(const xk_handle *h) {
  if (!h->d_R2 || !h->opt_slam_split || h->want_full_T) return 0;
  // 3: a SMALL stack -- a handful of tracks ended this frame (+ the SLAM rows): nominal rows <= n.  Not compressed either (the same branch of
  // vio_updater.cpp:487; the reference counts accepted rows, this counts nominal ones: it cannot wait for the verdicts): rows as built -> update.
  if (h->K + h->K2 > 0) {
    const long R = split_rows_nominal(h) + 2L * h->M;
    if (R <= std::min(h->n, h->CM)) return 3;
  }
  if (h->M <= 0) return 0;
  // 2: the stack is the SLAM features' rows and nothing else (no track ended this frame -- the common frame of a filter with persistent
  // features): 2 M rows against n > 3 M columns.  The reference compresses only when rows > columns (vio_updater.cpp:487); neither does this:
  // the rows go to the update as built, no QR launch at all (any n, any window).
  if (h->K + h->K2 == 0) return 2 * h->M <= h->CM ? 2 : 0;
  if (h->DB != 64 || !h->opt_resident || !h->persist_ok) return 0;
  if (h->n <= 206 || 6 * h->N + 1 > XkPipeWide::COLS) return 0;
  return pipe_queueable(h, split_rows_nominal(h), h->K + h->K2, pipe_rows_cap(6 * h->N + 1)) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
template <int RPL>
static void launch_merge(xk_handle *h, XkCaqrArgs &a, int groups, int csplit) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(xk_caqr_merge<RPL>), dim3(groups, csplit), dim3(16 * (16 + a.chalf)), 0, h->stream, a);
}

// The tile kernels (xk_caqr_tile, xk_caqr_fused) come in six variants <rows per lane, column range split over workgroups>: 16 rows next
// to 64-row slots; 26 next to 128-row slots whose tallest tile has <= 104 rows (two workgroups per CU, see xk_caqr_tile), else 32.
// f(rows per lane, split) gets them as integral constants.
template <typename F>
static void tile_variant(const xk_handle *h, int rows_max, int tsplit, F f) {
  auto with = [&](auto rpl) { tsplit == 1 ? f(rpl, std::false_type{}) : f(rpl, std::true_type{}); };
  if (h->DB == 64) with(std::integral_constant<int, 16>{});
  else if (rows_max <= 104 && h->opt_tall26) with(std::integral_constant<int, 26>{});
  else with(std::integral_constant<int, 32>{});
}
// per-tile kernel: 4 lanes per column, at most 192 (64-row tiles) / 128 (128-row tiles) columns per workgroup
static void tile_geom(const xk_handle *h, int c0, int &tsplit, int &tchalf, int &tthreads) {
  const int tile_cols = (h->DB == 64) ? 192 : 128;
  const int trail = std::max(0, h->C1 - c0 - 16);
  tsplit = std::max(1, (trail + (tile_cols - 16) - 1) / (tile_cols - 16));
  tchalf = (trail + tsplit - 1) / tsplit;
  tthreads = round_up(4 * (16 + tchalf), 64);
}
static void launch_tile(xk_handle *h, XkCaqrArgs &t) {
  int tsplit, tthreads;
  tile_geom(h, t.c0, tsplit, t.chalf, tthreads);
  const dim3 tgrid(t.ntiles, tsplit), tblock(tthreads);
  tile_variant(h, t.rows_max, tsplit, [&](auto rpl, auto split) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(xk_caqr_tile<decltype(rpl)::value, decltype(split)::value>), tgrid, tblock, 0, h->stream, t);
  });
}

// the runtime's verdict on the launches a schedule has queued
static int queued(xk_handle *h, const char *what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? XK_OK : fail(h, XK_EDEVICE, what, e);
}

// Arms a launch of xk_caqr_pipe over the pa.C1 columns of its system: the slab set and the sync words of this phase (the launch re-arms
// the other set for its successor), the test hooks, the tag of its accepted-rows word.
static int pipe_arm(xk_handle *h, XkCaqrPipeArgs &pa) {
  if (h->xsync_dirty) {
    // (a launch that gave up leaves its counters mid-count, its slabs half written and the other set half re-armed: arm both)
    if (hipMemsetAsync(h->d_xsync, 0, sizeof(unsigned) * 2 * XP_WORDS * 16, h->stream) != hipSuccess) return fail(h, XK_EDEVICE, "sync words");
    if (hipMemsetD32Async((hipDeviceptr_t)h->d_x1, (int)(XK_NOTYET_BITS & 0xffffffffu), 2 * 2 * h->xslab_doubles, h->stream) != hipSuccess) return fail(h, XK_EDEVICE, "slabs");
    h->xsync_dirty = false; h->xsync_phase = 0;
  }
  // (panels of THIS launch's system: the launch re-arms the other set by the same count, xk_caqr_pipe entry)
  const size_t np_ = (size_t)(pa.C1 + 15) / 16, strips_ = np_ * XK_PIPE_RLS, x1n = strips_ * 16 * h->C1P;
  double *set = h->d_x1 + (size_t)h->xsync_phase * h->xslab_doubles;
  pa.X1 = set; pa.X2 = set + x1n; pa.X1P = set + 2 * x1n;
  pa.Xnext = h->d_x1 + (size_t)(h->xsync_phase ^ 1) * h->xslab_doubles;
  pa.xnext_doubles = (long)h->xslab_doubles;
  pa.sync = h->d_xsync + (size_t)h->xsync_phase * XP_WORDS * 16;
  pa.sync_next = h->d_xsync + (size_t)(h->xsync_phase ^ 1) * XP_WORDS * 16;
  h->xsync_phase ^= 1;
  // test hook: raise the abort word before the launch -- every workgroup gives up at its first spin, exactly what an
  // uneven placement or a missing workgroup leads to, and the host has to redo the update with the multi-launch schedule
  if (h->opt_poison) {
    const unsigned seven = 7u;
    if (hipMemcpyAsync(pa.sync + XP_ABORT * 16, &seven, sizeof(unsigned), hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(h, XK_EDEVICE, "poison");
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, XK_EDEVICE, "poison");
  }
  pa.dbg = compress_env().persist_dbg ? h->d_pdbg : nullptr;
  pa.test_stall = h->opt_test_stall;
  h->pipe_tag = (h->pipe_tag % 0x7fff) + 1;               // 1 .. 32767: tags the accepted-rows word of THIS launch (eval_status)
  pa.acc_tag = h->pipe_tag;
  return XK_OK;
}

// The last columns [ccut, C1) of a tall system in ONE launch or TWO (xk_caqr_pipe<XkPipeTail> / <XkPipeTail4>): the rows of slots
// [slot0, slot0 + nslots) -- as the multi-launch schedule left them after the panels before ccut: R's rows zeroed where they were
// taken out, the leaders' first 32 rows holding merged rows -- plus `nextra` rows from behind the slots (the R of the launch before)
// are gathered into registers once, the panels run as in the single launch of the narrow systems, and rows ccut.. of R go to Rout
// (row stride C1P, column ccut at Rout[0]).
static int launch_pipe_tail(xk_handle *h, bool four, int ccut, int slot0, int nslots, int arity1, int nextra, double *Rout) {
  XkCaqrPipeArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.A = h->d_A + (size_t)slot0 * h->DB * h->C1P + ccut; pa.tile_rows = h->d_tile_rows + slot0; pa.nslots = nslots; pa.slot_rows = h->DB;
  pa.lead_stride = arity1;                        // (slot0 is a multiple of it)
  pa.nextra = nextra; pa.extra_row0 = (long)(h->ntiles_max - slot0) * h->DB;
  pa.Hc = nullptr; pa.hs = 0; pa.nhc = 0;
  pa.C1P = h->C1P; pa.C1 = h->C1 - ccut; pa.Rout = Rout; pa.S = h->d_rs; pa.PB = h->d_rpb;
  pa.status = h->d_status;
  { const int rca = pipe_arm(h, pa); if (rca != XK_OK) return rca; }
  h->pipe_rows_nominal = 0;                       // (the acceptance ratio belongs to the narrow geometries)
  if (four) hipLaunchKernelGGL(xk_caqr_pipe<XkPipeTail4>, dim3(h->n_cu), dim3(XK_PIPE_THREADS), 0, h->stream, pa);
  else hipLaunchKernelGGL(xk_caqr_pipe<XkPipeTail>, dim3(h->n_cu), dim3(XK_PIPE_THREADS), 0, h->stream, pa);
  return queued(h, "caqr tail launch");
}

// ---------------------------------------------------------------------------
// the schedules: each queues its work and, when that went through, writes `o` -- what launch_compress records in h->last -- once.
// (o comes in holding XK_SCHED_NONE and the `narrow2` of the last single launch, which only compress_single replaces.)
// ---------------------------------------------------------------------------
// no measurement rows at all: [T_H | z] = 0 (the reference skips the update, updater.cpp:106)
static int compress_none(xk_handle *h, XkOutcome &o) {
  if (hipMemsetAsync(h->d_R, 0, sizeof(double) * (size_t)h->C1P * h->C1P, h->stream) != hipSuccess) return fail(h, XK_EDEVICE, "R memset");
  o.schedule = XK_SCHED_EMPTY;
  return XK_OK;
}

// Rows that go to the update as built (split_plan 2 and 3): copied into d_R2, no QR launch at all.
static int compress_as_built(xk_handle *h, int mode, hipEvent_t mid, XkOutcome &o) {
  const size_t slam_bytes = sizeof(double) * 2 * (size_t)h->M * h->C1P;
  const double *slam_rows = h->d_A + (size_t)(h->K + h->K2) * h->DB * h->C1P;
  if (mode == 3) {
    // a small stack: tracks' rows by slot, MSCKF-SLAM tracks' behind them, then the SLAM rows
    const int Rt = h->K > 0 ? 2 * h->h_trk_off[h->K] - 3 * h->K : 0;   // (h_trk_off holds nothing when no track is staged)
    if (h->K > 0) hipLaunchKernelGGL(xk_stack_rows, dim3(h->K), dim3(256), 0, h->stream, h->d_A, h->d_tile_rows, h->d_trk_off, h->DB, h->C1P, 0, h->d_R2);
    if (h->K2 > 0)
      hipLaunchKernelGGL(xk_stack_rows, dim3(h->K2), dim3(256), 0, h->stream, h->d_A + (size_t)h->K * h->DB * h->C1P, h->d_tile_rows + h->K, h->d_trk2_off, h->DB,
                         h->C1P, Rt, h->d_R2);
    const long Rall = split_rows_nominal(h);
    if (h->M > 0 && hipMemcpyAsync(h->d_R2 + (size_t)Rall * h->C1P, slam_rows, slam_bytes, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      return fail(h, XK_EDEVICE, "SLAM rows");
    h->d_R2_dirty = true;                         // (rows below R1's diagonal and in the features' columns: the split compression never writes them)
  } else {
    // the SLAM rows alone (no track: K + K2 = 0, slot 0 is theirs), behind the 6 N rows a split compression would write
    if (hipMemcpyAsync(h->d_R2 + (size_t)6 * h->N * h->C1P, slam_rows, slam_bytes, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      return fail(h, XK_EDEVICE, "SLAM rows");
  }
  if (mid) hipEventRecord(mid, h->stream);
  o.schedule = mode == 3 ? XK_SCHED_SMALL_STACK : XK_SCHED_SLAM_ROWS;
  return queued(h, mode == 3 ? "stack rows" : "SLAM rows");
}

// The single launch (xk_caqr_pipe.hip.h): the whole stack into d_R or, sp, the split form -- the tracks' rows only, in the pose columns +
// the residual, into d_R2 (see xk_handle::d_R2).  Leaves o alone when the stack is not one it is queued for: the multi-launch schedule
// serves the update.  fuse: the Kalman update that follows; taken along where kalman_rides and the update is the plain one (sigma_img^2
// on every row, no external S, no range / sun rows), o.fused says so.
static int compress_single(xk_handle *h, int ntiles, bool sp, hipEvent_t mid, const UpdateSpec *fuse, XkOutcome &o) {
  const int C1s = sp ? 6 * h->N + 1 : h->C1, nslots_p = sp ? h->K + h->K2 : ntiles;
  const bool narrow = C1s <= XkPipeNarrow::COLS;
  const int R_nom = (int)split_rows_nominal(h) + (sp ? 0 : 2 * h->M);
  // two first-level groups per XCD when the rows expected to pass fit 152 tiles (2 % and half a tile's worth of margin); a launch
  // that finds more gives up at once (reason 9) and that geometry stays off for a while -- the 184-tile launch redoes the update
  bool split = false;
  if (narrow && h->opt_split > 0) {
    if (h->split_backoff > 0) --h->split_backoff;
    else if (h->opt_split >= 3) split = true;                              // (lab: always -- a stack that does not fit gives up, reason 9)
    else if (h->opt_split == 2) split = R_nom <= XkPipeNarrow2::ROWS;
    else if (h->acc_ratio > 0.0) split = (long)(h->acc_ratio * 1.02 * R_nom) + 64 <= XkPipeNarrow2::ROWS;
  }
  h->pipe_rows_nominal = R_nom;
  if (!pipe_queueable(h, R_nom, nslots_p, pipe_rows_cap(C1s))) return XK_OK;
  XkCaqrPipeArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.A = h->d_A; pa.tile_rows = h->d_tile_rows; pa.nslots = nslots_p; pa.slot_rows = 64;   // (no leaders, no extra rows: lead_stride = nextra = 0)
  pa.Hc = h->d_Hc; pa.hs = h->hc_stride; pa.nhc = h->rows_compact ? h->K : 0;
  pa.C1P = h->C1P; pa.C1 = C1s; pa.Rout = sp ? h->d_R2 : h->d_R; pa.S = h->d_rs; pa.PB = h->d_rpb;
  pa.res_col = sp ? h->na : 0;
  pa.status = h->d_status;
  { const int rca = pipe_arm(h, pa); if (rca != XK_OK) return rca; }
  pa.kal = 0; pa.kn = h->n; pa.Pin = nullptr; pa.Pout = nullptr; pa.sigma2 = 0.0; pa.corr = nullptr; pa.ct = nullptr; pa.done_flag = nullptr; pa.done_seq = 0;
  if (fuse && kalman_rides(h) && !fuse->S && !fuse->rdiag && !fuse->naux && fuse->T == h->d_R) {   // (T == d_R: not the split form, C1s = C1)
    // (a pass that leaves the covariance alone, cov_update = 0: the role needs the block-by-block posterior to get the
    //  correction right, so it runs as ever and its posterior goes to a scratch matrix; Pout becomes a copy of the prior below)
    pa.kal = 1; pa.Pin = fuse->Pin; pa.Pout = fuse->cov_update ? fuse->Pout : h->d_tmpP; pa.sigma2 = fuse->rscalar; pa.ct = fuse->ct;
    pa.corr = fuse->corr ? fuse->corr : h->d_corr;
    pa.done_flag = fuse->done_flag; pa.done_seq = fuse->done_seq;
  }
  if (sp && h->d_R2_dirty) {
    // the launch writes R1's upper trapezoid and the residual column only, and the update reads rows [0, 6 N) whole (u.tri = 0)
    if (hipMemsetAsync(h->d_R2, 0, sizeof(double) * (size_t)6 * h->N * h->C1P, h->stream) != hipSuccess) return fail(h, XK_EDEVICE, "R2 memset");
    h->d_R2_dirty = false;
  }
  if (split) hipLaunchKernelGGL(xk_caqr_pipe<XkPipeNarrow2>, dim3(h->n_cu), dim3(XK_PIPE_THREADS), 0, h->stream, pa);
  else if (narrow) hipLaunchKernelGGL(xk_caqr_pipe<XkPipeNarrow>, dim3(h->n_cu), dim3(XK_PIPE_THREADS), 0, h->stream, pa);
  else hipLaunchKernelGGL(xk_caqr_pipe<XkPipeWide>, dim3(h->n_cu), dim3(XK_PIPE_THREADS), 0, h->stream, pa);
  if (sp) {
    // the SLAM features' rows go into the compressed system as they were built: 2 M rows behind R1's 6 N (BEHIND the launch: row 6 N
    // of its output -- the residual column's own row of R, which nobody reads -- is the first of them)
    const int slam0 = h->K + h->K2;
    if (hipMemcpyAsync(h->d_R2 + (size_t)6 * h->N * h->C1P, h->d_A + (size_t)slam0 * h->DB * h->C1P, sizeof(double) * 2 * (size_t)h->M * h->C1P,
                       hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      return fail(h, XK_EDEVICE, "SLAM rows");
  }
  if (pa.kal && !fuse->cov_update && fuse->Pout != fuse->Pin &&
      hipMemcpyAsync(fuse->Pout, fuse->Pin, sizeof(double) * (size_t)h->n * h->n, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
    return fail(h, XK_EDEVICE, "prior copy");
  if (mid) hipEventRecord(mid, h->stream);
  const int NTP = 8 * (narrow ? (split ? XkPipeNarrow2::NT : XkPipeNarrow::NT) : XkPipeWide::NT);
  o = {sp ? XK_SCHED_SINGLE_SPLIT : XK_SCHED_SINGLE, pa.kal != 0, split, NTP, 1};
  return queued(h, "caqr launch");
}

// Tall systems: the LAST columns in one launch with every row in registers (xk_caqr_pipe<XkPipeTail>, xk_caqr_pipe.hip.h).  Like the single
// launch of the narrow systems it is queued on the nominal row count up to 5/4 of its capacity -- the launch counts the rows that passed
// the gates itself and gives up at once (reason 9) when they do not fit -- and only reads the stack: a tail that gives up is redone from
// the rows as they stand.
// ccut: first column the tail takes (a panel boundary; 0: no tail); half > 0: two launches, slots [0, half) then [half, ntiles) + the
// first one's R; four: the 4-lanes-per-column geometry (<= 192 columns)
struct XkTailPlan { int ccut, half; bool four; };
static XkTailPlan tail_plan(const xk_handle *h, int ntiles, int arity1, int groups1) {
  XkTailPlan p = {0, 0, false};
  // nominal rows of the slots before each group boundary; a leader's first 32 rows count whatever its slot holds
  std::vector<long> pre((size_t)groups1 + 1, 0);
  for (int g = 0; g < groups1; ++g) {
    long r = 0;
    for (int t = g * arity1; t < std::min(ntiles, (g + 1) * arity1); ++t) {
      const int v = slot_rows_nominal(h, t);
      r += (t % arity1 == 0) ? std::max(v, 32) : v;
    }
    pre[g + 1] = pre[g] + r;
  }
  const long R_nom = pre[groups1];
  if (R_nom < 64 * 8) return p;
  const int cc4 = 16 * std::max(1, (h->C1 - XkPipeTail4::COLS + 15) / 16), cc8 = 16 * ((h->C1 - XkPipeTail::COLS + 15) / 16);
  const int nx = h->C1 - cc4;                   // rows of the first launch's R
  int gh = 0;                                   // groups in the first half: the boundary that balances first half against second half + R
  for (int g = 1; g < groups1; ++g)
    if (std::labs(2 * pre[g] - R_nom - nx) < std::labs(2 * pre[gh] - R_nom - nx) || gh == 0) gh = g;
  const long capq = (long)XkPipeTail4::ROWS * 5 / 4;
  if (h->opt_tail != 2 && R_nom * 4 <= (long)XkPipeTail4::ROWS * 5) p = {cc4, 0, true};   // (the whole stack fits one 192-column launch)
  else if (h->opt_tail != 2 && gh > 0 && pre[gh] <= capq && R_nom - pre[gh] + nx <= capq) p = {cc4, gh * arity1, true};
  else if (cc8 >= 16 && R_nom * 4 <= (long)XkPipeTail::ROWS * 5) p = {cc8, 0, false};
  if (p.ccut >= h->C1) p.ccut = 0;
  return p;
}

// Overlapped multi-launch schedule (xk_caqr_fused): exactly two merge levels, the second one a single 20-way group whose launch also
// carries the tile step of the next panel.  tp.ccut > 0: the panels before ccut only, then the tail.  -> launches behind the first in *launches
static int multi_overlapped(xk_handle *h, XkCaqrArgs &a, int arity1, int groups1, const XkTailPlan &tp, hipEvent_t mid, int *launches) {
  const XkCompressEnv &env = compress_env();
  const int ntiles = a.ntiles;
  a.rows_max = std::max(a.rows_max, 32);        // a leader's pivot strip alternates between rows 0..15 and 16..31
  for (int c0 = 0, k = 0; c0 < h->C1; c0 += 16, ++k) {
    const int trail = std::max(0, h->C1 - c0 - 16);
    // last level inside the fused launch: 32 lanes per column next to 64-row tiles (768-thread workgroups),
    // 16 next to 128-row tiles (512-thread workgroups); whole waves either way
    // (2 trailing columns per workgroup next to 64-row tiles: 9 waves; measured 22.5 us per fused launch against
    //  23.4 at 4-8 columns -- the fewer waves share a step, the shorter it is, and there are CUs to spare)
    const int llanes = (h->DB == 64) ? 32 : 16;
    // (about 84 last-level workgroups at most: wider systems take more columns per workgroup)
    const int lauto = std::min(8, 2 * std::max(1, (trail + 2 * 84 - 1) / (2 * 84)));
    const int lchalf = (h->DB == 64) ? std::min(8, 2 * std::max(1, (env.lchalf ? env.lchalf : lauto) / 2))
                                     : std::min(16, 4 * std::max(1, (env.lchalf ? env.lchalf : 16) / 4));   // (16: config 3 418 -> 425 updates/s against 8, round 5 sweep)
    const int lsplit = std::max(1, (trail + lchalf - 1) / lchalf);
    const int lead_off = (k & 1) ? 16 : 0;
    if (k == 0) {
      XkCaqrArgs t = a;
      t.c0 = 0; t.stride = 1; t.final_level = 0; t.pin = nullptr; t.pout = h->d_panel[0];
      launch_tile(h, t);
      if (mid) hipEventRecord(mid, h->stream);
    }
    XkCaqrArgs m = a;                            // first level: leaders' pivot strips at lead_off, + the pending strips
    // columns per workgroup: at least `chalf`, and enough that groups x splits fits one workgroup per CU -- two
    // merge workgroups on a CU run ~1.6x longer than one (28.8 us at 420 workgroups, 17-19 us below 256)
    const int per_cu = std::max(1, env.cus / groups1);
    const int mchalf = env.adapt ? std::min(arity1 == 40 ? 16 : 32, std::max(env.chalf, 2 * ((trail + 2 * per_cu - 1) / (2 * per_cu)))) : env.chalf;
    const int msplit = std::max(1, (trail + mchalf - 1) / mchalf);
    m.c0 = c0; m.stride = 1; m.final_level = 0; m.pin = h->d_panel[0]; m.pout = h->d_panel[1]; m.chalf = mchalf;
    m.lead_off = lead_off; m.lead_all = 0; m.pend = (k > 0) ? 1 : 0;
    if (arity1 == 40 && env.m32) hipLaunchKernelGGL(xk_caqr_merge32, dim3(groups1, msplit), dim3(32 * (16 + mchalf)), 0, h->stream, m);
    else if (arity1 == 40) launch_merge<42>(h, m, groups1, msplit);
    else launch_merge<22>(h, m, groups1, msplit);
    ++*launches;
    XkCaqrArgs l = a;                            // last level: the leaders' pivot strips -> 16 rows of R
    l.c0 = c0; l.stride = arity1; l.final_level = 1; l.pin = h->d_panel[1]; l.pout = h->d_panel[0]; l.chalf = lchalf;
    l.lead_off = lead_off; l.lead_all = 1; l.pend = 0;
    if (tp.ccut > 0 && c0 + 16 == tp.ccut) {
      // the last panel of the multi-launch part: its last level alone, then the tail launch takes the stack as it stands
      launch_merge<20>(h, l, 1, lsplit);
      ++*launches;
      const int ccut = tp.ccut;
      double *const Rtail = h->d_R + (size_t)ccut * h->C1P + ccut;   // rows ccut.. of R, column ccut first
      int rct;
      if (tp.half > 0) {
        double *Ra = h->d_A + (size_t)h->ntiles_max * h->DB * h->C1P + ccut;           // the first launch's R: behind the slots
        rct = launch_pipe_tail(h, true, ccut, 0, tp.half, arity1, 0, Ra);
        if (rct == XK_OK) rct = launch_pipe_tail(h, true, ccut, tp.half, ntiles - tp.half, arity1, h->C1 - ccut, Rtail);
        ++*launches;
      } else rct = launch_pipe_tail(h, tp.four, ccut, 0, ntiles, arity1, 0, Rtail);
      if (rct != XK_OK) return rct;
      ++*launches;
      break;
    }
    if (c0 + 16 < h->C1) {
      XkCaqrArgs t = a;                          // ... next to the tile step of the next panel
      t.c0 = c0 + 16; t.stride = 1; t.final_level = 0; t.pin = nullptr; t.pout = h->d_panel[0];
      t.hole_stride = arity1; t.lead_off = 16 - lead_off;
      int tsplit, tthreads;
      tile_geom(h, t.c0, tsplit, t.chalf, tthreads);
      const dim3 grid(lsplit + ntiles * tsplit), block(std::max(tthreads, round_up(llanes * (16 + lchalf), 64)));
      tile_variant(h, t.rows_max, tsplit, [&](auto rpl, auto split) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(xk_caqr_fused<decltype(rpl)::value, decltype(split)::value>), grid, block, 0, h->stream, t, l, lsplit, tsplit);
      });
    } else {
      launch_merge<20>(h, l, 1, lsplit);
    }
    ++*launches;
  }
  return XK_OK;
}

// Multi-launch schedule level by level: per panel the tile step, then merge levels until one strip is left.  -> launches behind the first
static int multi_by_level(xk_handle *h, XkCaqrArgs &a, int arity1, hipEvent_t mid) {
  const int ntiles = a.ntiles;
  int launches = 0;
  for (int c0 = 0; c0 < h->C1; c0 += 16) {
    const int trail = std::max(0, h->C1 - c0 - 16);
    a.c0 = c0; a.stride = 1; a.final_level = 0; a.pin = nullptr; a.pout = h->d_panel[0];
    launch_tile(h, a);
    if (c0 == 0 && mid) hipEventRecord(mid, h->stream);
    if (c0 > 0) ++launches;                                        // (the first tile launch is timed as its own stage)
    a.chalf = compress_env().chalf;
    const int csplit = std::max(1, (trail + a.chalf - 1) / a.chalf);
    int stride = 1, level = 0;
    do {
      const int left = (ntiles + stride - 1) / stride;             // strips still alive at this level
      const int arity = (stride == 1) ? arity1 : (left > 20 ? 40 : 20);
      a.stride = stride;
      a.final_level = (left <= arity) ? 1 : 0;
      const int groups = (left + arity - 1) / arity;
      a.pin = h->d_panel[level & 1];
      a.pout = h->d_panel[(level + 1) & 1];
      ++level;
      if (arity == 40) launch_merge<40>(h, a, groups, csplit);
      else launch_merge<20>(h, a, groups, csplit);
      ++launches;
      stride *= arity;
    } while (stride < ntiles);
  }
  return launches;
}

// The multi-launch CAQR of the whole stack into d_R, panels of 16 columns (d_R was zeroed at creation; the merges rewrite the whole
// upper trapezoid every update and nothing else): overlapped where two merge levels cover the stack, with the tail where it is armed
// and the rows fit, level by level otherwise.
static int compress_multi(xk_handle *h, int ntiles, hipEvent_t mid, XkOutcome &o) {
  const XkCompressEnv &env = compress_env();
  XkCaqrArgs a;
  memset(&a, 0, sizeof(a));
  a.A = h->d_A; a.tile_rows = h->d_tile_rows; a.ntiles = ntiles; a.TS = h->DB;
  a.C1P = h->C1P; a.C1 = h->C1; a.Rout = h->d_R; a.dbg = nullptr;
  a.wt = env.wt;
  {   // tallest tile: 2 L_max - 3 rows for the track tiles, full slots for packed SLAM rows
    const int lmax = std::max(h->K > 0 ? h->h_pin_i[0] : 0, h->K2 > 0 ? h->h_pin_i[1] : 0);
    a.rows_max = (h->M > 0) ? h->DB : std::min(h->DB, std::max(16, 2 * lmax - 3));
  }
  // first-level arity: 40 strips per workgroup once 20 x 20 no longer covers the stack in two levels
  const int arity1 = env.arity1 ? env.arity1 : (ntiles > 400 ? 40 : 20);
  const int groups1 = (ntiles + arity1 - 1) / arity1;
  const bool overlap = env.overlap && (arity1 == 20 || arity1 == 40) && groups1 >= 2 && groups1 <= 20;
  a.hole_stride = 0; a.lead_off = 0; a.lead_all = 0; a.pend = 0;
  a.lead_stride = env.skip_rejected ? arity1 : 0;
  // (the tiles of the tracks may be factor records: the first tile pass below forms its rows from them and leaves tiles behind)
  a.Hc = h->d_Hc; a.hs = h->hc_stride; a.hcvr = xk_hc_vr(h->DB); a.nhc = (h->rows_compact && h->K > 0) ? h->K : 0;
  h->rows_compact = false;
  // the tail: re-armed after `rearm_after` clean updates like the fast path; off while it backs off from an overflow (reason 9)
  const bool tail_wanted = h->opt_resident && h->opt_tail;
  const bool tail_rearmable = h->tail_capable && !h->tail_ok && tail_wanted && h->rearm_after > 0 && h->tail_backoff == 0;
  if (tail_rearmable) {
    ++h->tail_clean;                              // one more update the multi-launch schedule served alone
    if (h->tail_clean > h->rearm_after) { h->tail_ok = true; h->tail_clean = 0; }
  }
  XkTailPlan tp = {0, 0, false};
  if (h->tail_backoff > 0) --h->tail_backoff;
  else if (overlap && h->tail_ok && tail_wanted && ntiles <= XK_PIPE_SLOTS_MAX) tp = tail_plan(h, ntiles, arity1, groups1);
  int launches = 0;
  if (overlap) {
    const int rc = multi_overlapped(h, a, arity1, groups1, tp, mid, &launches);
    if (rc != XK_OK) return rc;
  } else launches = multi_by_level(h, a, arity1, mid);
  o = {tp.ccut > 0 ? XK_SCHED_MULTI_TAIL : XK_SCHED_MULTI, false, o.narrow2, ntiles, launches};
  return queued(h, "caqr launch");
}

// QR compression of the staged tile stack (vio_updater.cpp:487-512), or what stands in for it: picks the schedule and records what it
// left in h->last.  mid: (optional) recorded behind the first launch (xk_bench_staged's stage boundary).
// fuse: (optional) the Kalman update that follows this compression.  If the single launch takes it along (narrow geometry,
// correction_total = 0, covariance update, no external S), h->last.fused says so and the caller must NOT queue launch_update.
static int launch_compress(xk_handle *h, hipEvent_t mid = nullptr, const UpdateSpec *fuse = nullptr) {
  if (h->upd.stage == XK_UPD_STAGED) return fail(h, XK_EINVAL, "xk_msckf_build has not run on the staged inputs");
  const int slam_tiles = (2 * h->M + h->DB - 1) / h->DB;
  const int ntiles = h->K + h->K2 + slam_tiles;
  const int mode = h->want_full_T ? 0 : h->plan;   // (latched at the build: what compressed_spec saw; xk_qr_compress: the whole stack)
  XkOutcome o = {};
  o.narrow2 = h->last.narrow2;
  int rc;
  if (ntiles == 0) rc = compress_none(h, o);
  else if (mode >= 2) rc = compress_as_built(h, mode, mid, o);
  else {
    // (ntiles > 0 here, so the stack has a track or a SLAM row -- slam_tiles > 0 iff M > 0: the old `fast_shape` conjunct of the two
    //  tests below was always true and is gone)
    // the fast path steps back in after `rearm_after` clean multi-launch updates (the sync words of the launch that gave up: pipe_arm)
    const bool rearmable = h->opt_resident && !h->persist_ok && h->fast_capable && h->rearm_after > 0;
    if (rearmable) {
      ++h->clean_classic;                         // one more update since the give-up that the single launch did not serve
      if (h->clean_classic > h->rearm_after) { h->persist_ok = true; h->clean_classic = 0; }
    }
    rc = (h->opt_resident && h->persist_ok) ? compress_single(h, ntiles, mode == 1, mid, fuse, o) : XK_OK;
    if (rc == XK_OK && o.schedule == XK_SCHED_NONE) rc = compress_multi(h, ntiles, mid, o);
  }
  if (rc != XK_OK) return rc;
  h->last = o;
  // A compression that xk_build_compress_async left for xk_apply_update is no longer deferred once ANY compression has run: an
  // xk_qr_compress in between does the work now, and xk_apply_update then applies d_R as it stands instead of compressing rows the
  // multi-launch schedule has already reduced in place.  (A queued pass stays queued.)
  if (h->upd.stage < XK_UPD_COMPRESSED) h->upd.stage = XK_UPD_COMPRESSED;
  return XK_OK;
}

// ---------------------------------------------------------------------------
// the system the compression leaves for the update
// ---------------------------------------------------------------------------
static UpdateSpec compressed_spec_base(xk_handle *h, const double *d_ct, int cov_update) {
  UpdateSpec u;
  memset(&u, 0, sizeof(u));
  u.str = h->C1P; u.stc = 1; u.kdim = h->na; u.col0 = XK_CORE; u.sz = h->C1P;   // rows of C1P doubles over the active columns, the residual at column na
  u.rdiag = nullptr; u.rscalar = h->sigma_img * h->sigma_img;    // vio_updater.cpp:508-509; the SLAM rows carry sigma_img^2 too (slam_update.cpp: r = var_img I)
  u.Pin = h->d_P; u.Pout = h->d_Pout; u.ct = d_ct; u.cov_update = cov_update;
  if (const int mode = h->upd.stage >= XK_UPD_COMPRESSED ? outcome_R2_mode(h->last) : h->plan) {
    // the split form (d_R2): 6 N rows of R1 over the pose columns, then the 2 M rows of the SLAM features as built; mode 2: those rows alone
    const int r0 = mode == 2 ? 6 * h->N : 0;
    u.T = h->d_R2 + (size_t)r0 * h->C1P;
    u.c = mode == 3 ? (int)split_rows_nominal(h) + 2 * h->M : 6 * h->N + 2 * h->M - r0;   // (3: every track's rows, then the SLAM rows)
    u.tri = 0;                                     // (the SLAM rows are not below anybody's diagonal)
  } else {
    u.T = h->d_R; u.c = h->na;                     // R[0], rows 0..na-1
    u.tri = 1;                                     // d_R: zero below the diagonal (zeroed at creation, only the trapezoid is ever written)
  }
  u.z = u.T + h->na;
  return u;
}
static UpdateSpec compressed_spec(xk_handle *h, const double *d_ct, int cov_update) {
  UpdateSpec u = compressed_spec_base(h, d_ct, cov_update);
  if (h->naux > 0) {
    u.naux = h->naux;
    if (h->K + h->K2 + h->M == 0) u.c = 0;        // (no visual row at all: the update is the range / sun rows alone)
  }
  return u;
}

// ---------------------------------------------------------------------------
// status words
// ---------------------------------------------------------------------------
#define XK_RETRY_CLASSIC 1000   // internal: the single-launch CAQR gave up, the multi-launch schedule must redo the update
// how every give-up ends: counted, the sync words to be cleared, the rows to be rebuilt (h->err already says why)
static int give_up(xk_handle *h, int pst, bool allow_retry) {
  h->fast_giveups++; h->fast_reason = pst;
  h->xsync_dirty = true;
  pending_drop(h);
  return allow_retry ? XK_RETRY_CLASSIC : XK_EDEVICE;
}
static int eval_status(xk_handle *h, int st, int pst, bool allow_retry) {
  const bool tail = h->last.schedule == XK_SCHED_MULTI_TAIL;
  // What the last single launch found (status word 2): accepted rows in the low 15 bits, the launch's tag above them.  The word is a
  // relaxed system-scope store of a tile workgroup, not ordered with the completion marker (another workgroup's store): a count that
  // carries another launch's tag is a late arrival and is left alone -- it must not be divided by THIS launch's nominal rows.
  if ((outcome_single(h->last) || tail) && h->pipe_rows_nominal > 0) {   // (a launch of xk_caqr_pipe ended the compression)
    const int w2 = h->d_status[2];
    if (w2 > 0 && (w2 >> 15) == h->pipe_tag) h->acc_ratio = (double)(w2 & 0x7fff) / h->pipe_rows_nominal;
  }
  if (pst == 0 && tail) h->tail_backoff_len = 64;      // (a tail that ran through: the next overflow starts at 64 updates off again)
  if (st != 0 || pst != 0) {
    hipStreamSynchronize(h->stream);
    h->d_status[0] = h->d_status[1] = 0;
  }
  if (pst != 0) {
    // reasons: 1 grid not resident, 2 XCD barrier, 3 uneven XCD placement, 4/5 waiting for the last / first level
    // The fast path steps aside, but not for the life of the handle: after `rearm_after` clean multi-launch updates it is
    // tried again (the other tenant of the GPU may be gone); every further give-up doubles that distance, so a permanently
    // shared GPU costs one bounded retry (<= 2 ms, xk_spin_ge) every few thousand updates at most.
    const bool again = h->fast_giveups >= 1;     // not the first give-up of this handle
    if (tail) {
      // the tail launch of a tall system gave up: it only READ the stack, but the retry below rebuilds the rows anyway (one code path);
      // reason 9 = more rows passed the gates than its tiles hold -- off for the next 64 updates; anything else = co-residency
      if (pst == 9) { h->tail_backoff = std::max(64, h->tail_backoff_len); h->tail_backoff_len = std::min(4096, 2 * std::max(64, h->tail_backoff_len)); }
      else { h->tail_ok = false; h->tail_clean = -1; if (again) h->rearm_after = std::min(4096, std::max(1, h->rearm_after) * 2); }
      snprintf(h->err, sizeof(h->err), "single-launch CAQR tail gave up (reason %d); the multi-launch schedule finishes the factorisation", pst);
    } else if (pst == 9 && h->last.narrow2) {
      // the 152-tile geometry was chosen on the LAST update's acceptance ratio and this update passed more: not a co-residency
      // problem and not a capacity cliff of the fast path -- the 184-tile launch redoes the update, the split geometry stays off
      // for the next 64 updates
      h->split_backoff = 64;
      snprintf(h->err, sizeof(h->err), "single-launch CAQR (152 tiles): more rows passed the gates than expected; redone with 184 tiles");
    } else if (pst == 9) {
      // not a co-residency problem: more rows passed the gates than the tiles of the single launch hold.  The fast path stays
      // armed for smaller stacks; this size goes to the multi-launch schedule from now on.
      h->overflow_rows = h->overflow_rows ? std::min(h->overflow_rows, h->pipe_rows_nominal) : h->pipe_rows_nominal;
      snprintf(h->err, sizeof(h->err), "single-launch CAQR: %d nominal rows held more accepted rows than its tiles; multi-launch schedule from that size on", h->pipe_rows_nominal);
    } else {
      h->persist_ok = false;
      h->clean_classic = -1;                      // (-1: the retry of THIS update is not a clean update)
      if (again) h->rearm_after = std::min(4096, std::max(1, h->rearm_after) * 2);
      snprintf(h->err, sizeof(h->err), "single-launch CAQR gave up (reason %d): workgroups not co-resident; multi-launch schedule for the next %d updates", pst, h->rearm_after);
    }
    return give_up(h, pst, allow_retry);
  }
  if (st != 0) return fail(h, st, "innovation covariance not positive definite");
  return XK_OK;
}
static int read_status(xk_handle *h, bool allow_retry = false) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  stage_stream_idle(h);
  return eval_status(h, h->d_status[0], h->d_status[1], allow_retry);
}
