// xk_update_api.hip.h -- host side of the filter's update path: the launches that build the rows, compress them (xk_compress.hip.h,
// included below where its kernels have always stood) and apply the Kalman update; the one pass every entry queues and its redo after a
// single launch that gave up; the staged and queued entries, xk_apply_update, the dense update, xk_bench_staged and xk_run_steps.  How far
// the staged update has got is kept in xk_handle::upd (xk_handle.hip.h).  Part of xk_api.hip's translation unit, included behind the
// staging helpers and the covariance entries.
#pragma once

// ---------------------------------------------------------------------------
// launch helpers (all asynchronous on h->stream)
// ---------------------------------------------------------------------------

static int split_plan(const xk_handle *h);
static long split_rows_nominal(const xk_handle *h);

// The range / sun rows of this update (xk_aux.hip.h), queued behind the per-feature kernels: one workgroup, no host synchronisation.
// Their variances follow the REFERENCE's stack, not this engine's schedule: the reference compresses when its rows -- every MSCKF and
// MSCKF-SLAM track's 2 L - 3, the SLAM features' 2 M, 1 range row, 2 sun rows, accepted or not -- exceed n + 1
// (vio_updater.cpp:487-490), and then gives EVERY row sigma_img^2 (:507-509): a compressed range row weighs as if sigma_range were
// sigma_img.  Uncompressed, each row keeps its own: sigma_range^2 (1 for a gated-out row), var_sun.
static int launch_aux(xk_handle *h, double sigma_img) {
  XkAuxIn in = h->aux_in;
  in.has_range = (h->aux_mask & 1) ? 1 : 0;
  in.has_sun = (h->aux_mask & 2) ? 1 : 0;
  if (in.has_range) {
    if (h->M < 3) return fail(h, XK_EINVAL, "range row: fewer than 3 SLAM features staged");
    for (int j = 0; j < 3; ++j)
      if (in.facet[j] >= h->M) return fail(h, XK_EINVAL, "range row: facet feature id outside the staged SLAM features");
  }
  const long nominal = split_rows_nominal(h) + 2L * h->M + h->naux;
  in.compressed = nominal > (long)h->n + 1 ? 1 : 0;
  in.var_comp = sigma_img * sigma_img;
  in.chi1 = XK_CHI2_090[1];
  XkAuxArgs a;
  a.q = h->d_q; a.p = h->d_p; a.n_poses = h->n_poses; a.N = h->N;
  a.feat = h->d_feat; a.anchor = h->d_anchor; a.P = h->d_P; a.n = h->n;
  a.in = in;                                      // (by value: no host-to-device copy, no staging slot, replays included)
  a.rows = h->d_aux;
  a.rdiag = a.rows + 3 * ((size_t)h->n + 1);
  a.flags = a.rdiag + 3;
  hipLaunchKernelGGL(xk_aux_rows, dim3(1), dim3(XK_AUX_THREADS), 0, h->stream, a);
  return XK_OK;
}

// replay: the build of an update that is being redone (a retry) or repeated (xk_run_steps / xk_bench_staged past the first step) -- the
// range / sun rows of that update are built again; any other build takes what has been staged since the last one (possibly nothing).
static int launch_build(xk_handle *h, double sigma_img, bool replay = false) {
  if (h->n_poses < 2) return fail(h, XK_EINVAL, "window not staged");
  if (h->K > 0 && h->h_pin_i[0] > h->n_poses) return fail(h, XK_EINVAL, "track longer than the staged window");
  const int slam_tiles = (2 * h->M + h->DB - 1) / h->DB;
  XkFeatArgs fa;
  memset(&fa, 0, sizeof(fa));
  size_t feat_lds = 0;
  { int rcw = flush_window(h); if (rcw != XK_OK) return rcw; }   // (normally carried by the frame's congruence launch already)
  h->plan = split_plan(h);
  outcome_release_R2(h->last);                    // (d_R2 holds nothing of THIS update until launch_compress writes it)
  if (h->K > 0) {
    XkFeatArgs &a = fa;
    a.q = h->d_q; a.p = h->d_p; a.n_poses = h->n_poses; a.n_poses_max = h->N;
    a.trk_off = h->d_trk_off; a.obs = h->d_obs; a.K = h->K;
    a.P = h->d_P; a.n = h->n; a.var_img = sigma_img * sigma_img; a.chi95 = h->d_chi95;
    a.A = h->d_A; a.DB = h->DB; a.C1P = h->C1P; a.na = h->na;
    // factor records instead of tiles: H0 never visits HBM.  Whoever compresses forms its rows from them -- the tile workgroups
    // of the single launch (narrow systems; next to the wide geometry's 80-row tiles and 2 lanes per column forming the entries
    // costs more than the tiles' trip through HBM -- config 2: 1546 -> 1521 updates/s -- so those keep their tiles), or the
    // first pass of the multi-launch schedule (128-row slots: always; 64-row slots: when the single launch was armed and then
    // not taken or gave up).
    h->rows_compact = h->opt_hlite && h->d_Hc && !h->feat_dbg && h->plan != 3 &&      // (an uncompressed small stack is copied from tiles)
                      (h->DB == 128 || (h->opt_resident && h->persist_ok && (h->C1 <= XkPipeNarrow::COLS || h->opt_hlite >= 2)));   // (lab: 2 = the wide geometry too)
    a.Hc = h->rows_compact ? h->d_Hc : nullptr; a.hs = h->hc_stride; a.hcvr = xk_hc_vr(h->DB);
    a.tile_rows = h->d_tile_rows; a.inlier = h->d_inl; a.gamma = h->d_gam; a.gpf = h->d_gpf; a.gn_iters = h->d_gn;
    a.gpf_in = nullptr; a.up_out = nullptr; a.batch = nullptr; a.dbg = h->feat_dbg; a.gate_form = h->opt_gate_form;
    a.inlier_h = h->h_flag_i; a.gamma_h = h->h_flag_d;     // gate results also straight into the pinned flag cache
    const bool packed = xk_feature_packed(h->n_poses);      // windows of more than 33 poses: gate matrix as a packed triangle
    feat_lds = xk_feature_lds_bytes(h->n_poses, packed);
    // (with SLAM features the tracks and the features share one launch, below)
    if (packed) hipLaunchKernelGGL(xk_msckf_feature_packed, dim3(h->K), dim3(XK_FEAT_THREADS), feat_lds, h->stream, a);
    else if (h->M == 0 || h->feat_dbg) hipLaunchKernelGGL(xk_msckf_feature, dim3(h->K), dim3(XK_FEAT_THREADS), feat_lds, h->stream, a);
  }
  if (h->K2 > 0) {   // tracks that become persistent features this frame: tiles K .. K + K2 - 1
    if (h->h_pin_i[1] > h->n_poses) return fail(h, XK_EINVAL, "MSCKF-SLAM track longer than the staged window");
    XkTriMultiArgs ta{h->d_q, h->d_p, h->d_obs2, 0, h->d_gpf2, h->d_gn2, h->d_trk2_off, h->n_poses};
    hipLaunchKernelGGL(xk_triangulate_multi, dim3(h->K2), dim3(64), 0, h->stream, ta);
    XkSlamInitArgs a;
    a.q = h->d_q; a.p = h->d_p; a.n_poses = h->n_poses; a.n_poses_max = h->N;
    a.trk_off = h->d_trk2_off; a.obs = h->d_obs2; a.gpf = h->d_gpf2;
    a.P = h->d_P; a.n = h->n; a.na = h->na; a.var_img = sigma_img * sigma_img; a.chi95 = h->d_chi95;
    a.A = h->d_A + (size_t)h->K * h->DB * h->C1P; a.DB = h->DB; a.C1P = h->C1P; a.W = h->d_W2;
    a.tile_rows = h->d_tile_rows + h->K; a.inlier = h->d_inl2; a.gamma = h->d_gam2;
    a.H1 = h->d_H1; a.H2 = h->d_H2; a.r1 = h->d_r1; a.features = h->d_feat2;
    const size_t lds = xk_slaminit_lds_bytes(h->n_poses);
    if (!h->attr_slaminit) {   // per handle = per device: a process may hold handles on several GPUs
      hipFuncSetAttribute((const void *)xk_msckf_slam_init, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
      h->attr_slaminit = true;
    }
    hipLaunchKernelGGL(xk_msckf_slam_init, dim3(h->K2), dim3(XK_FEAT_THREADS), lds, h->stream, a);
    h->ms_built = true;
  }
  if (h->M > 0) {
    if (h->anchor_max >= h->n_poses) return fail(h, XK_EINVAL, "SLAM anchor outside the staged window");
    XkSlamArgs s;
    s.q = h->d_q; s.p = h->d_p; s.n_poses = h->n_poses; s.n_poses_max = h->N;
    s.feat = h->d_feat; s.anchor_idxs = h->d_anchor; s.z_last = h->d_zlast; s.M = h->M;
    s.P = h->d_P; s.n = h->n; s.var_img = sigma_img * sigma_img; s.chi = h->d_chi_s;
    s.A = h->d_A + (size_t)(h->K + h->K2) * h->DB * h->C1P; s.DB = h->DB; s.C1P = h->C1P; s.na = h->na;
    s.inlier = h->d_inl_s; s.gamma = h->d_gam_s;
    if (h->K > 0 && !h->feat_dbg && !xk_feature_packed(h->n_poses)) hipLaunchKernelGGL(xk_build_rows, dim3(h->K + h->M), dim3(XK_FEAT_THREADS), feat_lds, h->stream, fa, s);
    else hipLaunchKernelGGL(xk_slam_rows, dim3(h->M), dim3(64), 0, h->stream, s);
    // rows per SLAM tile (gated-out features leave zero rows, as in the reference)
    for (int t = 0; t < slam_tiles; ++t) h->h_pin_i[8 + t] = std::min(h->DB, 2 * h->M - t * h->DB);
    if (hipMemcpyAsync(h->d_tile_rows + h->K + h->K2, h->h_pin_i + 8, sizeof(int) * slam_tiles, hipMemcpyHostToDevice,
                       h->stream) != hipSuccess)
      return fail(h, XK_EDEVICE, "tile_rows upload");
  }
  if (h->aux_staged || !replay) {                  // (a replay keeps the rows of the update it repeats)
    h->aux_mask = h->aux_staged;
    h->aux_staged = 0;
  }
  h->naux = ((h->aux_mask & 1) ? 1 : 0) + ((h->aux_mask & 2) ? 2 : 0);
  if (h->naux) { int rca = launch_aux(h, sigma_img); if (rca != XK_OK) return rca; }
  h->sigma_img = sigma_img;
  pending_drop(h);                                 // (a build starts the update over: whatever was compressed, deferred or queued before it is abandoned)
  h->upd.stage = XK_UPD_ROWS;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, XK_EDEVICE, "build launch", e);
  return XK_OK;
}

// ---------------------------------------------------------------------------
// compression of the staged rows: schedules, the system they leave for the update, status words
// ---------------------------------------------------------------------------
#include "xk_compress.hip.h"

static void gemm(xk_handle *h, const XkGemmArgs &g) {
  const int tiles = xk_gemm_grid(g);
  if (tiles <= 0) return;
  hipLaunchKernelGGL(xk_gemm_f64, dim3(tiles), dim3(64 * XK_GEMM_WAVES), 0, h->stream, g);
}

// Kalman algebra on the device (updater.cpp:117-141 / :144-161).
static int launch_update(xk_handle *h, const UpdateSpec &u_in) {
  UpdateSpec u = u_in;
  if (u.naux > 0) {
    // the range / sun rows join the system as built (they never go through the QR): [T ; H_aux]^T [T ; H_aux] is the Gram matrix of the
    // whole stack, and the same for the residual -- the argument of the split form for the SLAM rows.  The sun rows touch core columns
    // 6..8, so the system is widened to all n columns, with one variance per row (xk_aux.hip.h chose the rows' own).
    if (u.c + u.naux > h->CM) return fail(h, XK_ECAPACITY, "measurement rows exceed workspace");
    XkAuxStackArgs s;
    s.T = u.T; s.str = u.str; s.stc = u.stc; s.c = u.c; s.kdim = u.kdim; s.col0 = u.col0;
    s.z = u.z; s.sz = u.sz; s.rdiag = u.rdiag; s.rscalar = u.rscalar;
    s.aux = h->d_aux; s.aux_rdiag = s.aux + 3 * ((size_t)h->n + 1); s.naux = u.naux;
    s.n = h->n; s.out = h->d_Taug; s.out_rdiag = h->d_Taug + (size_t)h->CM * (h->n + 1);
    hipLaunchKernelGGL(xk_aux_stack, dim3(u.c + u.naux), dim3(256), 0, h->stream, s);
    u.T = s.out; u.str = h->n + 1; u.stc = 1; u.c += u.naux; u.kdim = h->n; u.col0 = 0;
    u.z = s.out + h->n; u.sz = h->n + 1; u.rdiag = s.out_rdiag; u.tri = 0; u.naux = 0;
  }
  const int c = u.c, n = h->n, LDA = h->LDA;
  if (c <= 0 || c > h->CM) return fail(h, XK_ECAPACITY, "measurement rows exceed workspace");
  XkGemmArgs g;
  memset(&g, 0, sizeof(g));
  // W = T * Pin[col0:col0+kdim, :]                      (H P)
  g.A = u.T; g.sar = u.str; g.sac = u.stc;
  g.B = u.Pin + u.col0; g.sbr = 1; g.sbc = n;
  g.C = h->d_Maug + c; g.scr = LDA; g.scc = 1;
  g.D = g.C; g.sdr = LDA; g.sdc = 1;
  g.M = c; g.N = n + 1; g.K = u.kdim; g.alpha = 1.0; g.beta = 0.0; g.mode = 0;
  static const int struct_env = env_int("XK_GEMM_STRUCT", 1);   // 0: every product as a general one (A/B switch)
  g.tri_a = struct_env && u.tri;
  // extra column: z' = res + H corr_tot  (updater.cpp:126) lands next to W in the augmented matrix
  g.xcol = 1; g.bx = u.ct ? u.ct + u.col0 : nullptr; g.sbx = 1; g.dx = u.z; g.sdx = u.sz;
  g.cx = h->d_Maug + c + n; g.scx = LDA;
  gemm(h, g);
  if (u.S) {
    XkCopyArgs cp{u.S, h->d_Maug, c, c, u.ssr, u.ssc, (long)LDA, 1};
    hipLaunchKernelGGL(xk_copy2d, dim3((c * c + 255) / 256), dim3(256), 0, h->stream, cp);
  } else {
    // S = W[:, col0:col0+kdim] * T^T + R               (H P H^T + R)
    memset(&g, 0, sizeof(g));
    g.A = h->d_Maug + c + u.col0; g.sar = LDA; g.sac = 1;
    g.B = u.T; g.sbr = u.stc; g.sbc = u.str;
    g.C = h->d_Maug; g.scr = LDA; g.scc = 1;
    g.D = g.C; g.sdr = LDA; g.sdc = 1;
    g.M = c; g.N = c; g.K = u.kdim; g.alpha = 1.0; g.beta = 0.0; g.mode = 1;
    g.tri_b = struct_env && u.tri;
    g.sym_cols = struct_env ? c : 0;   // only the upper triangle of S is read (xk_chol_whole / xk_chol_step)
    g.diag = u.rdiag; g.diag_scalar = u.rscalar;
    gemm(h, g);
  }
  // blocked Cholesky with the right-hand sides carried along: one launch per 32-column block step
  const int ncols = c + n + 1;
  static const int whole_env = env_int("XK_CHOL_WHOLE", 1);
  static const int split_env = env_int("XK_CHOL_SPLIT", 1);
  if (whole_env && (c <= 16 * XK_CHOLW_MAXB || split_env)) {
    // Every block step inside one launch (xk_chol_whole), one workgroup per 16 right-hand-side columns.  Systems with
    // more than 192 rows (BASELINE configs 2 and 3: c = 331 / 301) are cut into 192-row slabs:
    //   X[0:b, b:]  = L_11^-1 [S_12 | W_1 | z_1]        xk_chol_whole on the slab, the rest of ITS ROWS as right-hand sides
    //   M[b:, b:]  -= X[0:b, b:c]^T X[0:b, b:]           one fp64-MFMA GEMM (Schur complement of S and of the right-hand sides)
    // and the remainder is the same problem again: 2 slabs = 3 launches instead of 11 block-step launches.
    const int B = 16 * XK_CHOLW_MAXB;
    for (int off = 0; off < c;) {
      const int cb = std::min(B, c - off);
      XkCholWholeArgs d;
      d.Maug = h->d_Maug + (size_t)off * LDA + off; d.ld = LDA; d.c = cb; d.ncols = ncols - off;
      d.X = h->d_X + (size_t)off * LDA + off; d.status = h->d_status;
      xk_cholw_table((cb + 15) / 16, d.tab);
      hipLaunchKernelGGL(xk_chol_whole, dim3((ncols - off - cb + 15) / 16), dim3(64 * XK_CHOLW_WAVES), 0, h->stream, d);
      off += cb;
      if (off < c) {
        XkGemmArgs s;
        memset(&s, 0, sizeof(s));
        const double *Xs = h->d_X + (size_t)(off - cb) * LDA + off;       // X[slab rows, off:]
        s.A = Xs; s.sar = 1; s.sac = LDA;                                   // A[i][k] = X[k][off + i]
        s.B = Xs; s.sbr = LDA; s.sbc = 1;                                   // B[k][j] = X[k][off + j]
        s.C = h->d_Maug + (size_t)off * LDA + off; s.scr = LDA; s.scc = 1;
        s.D = s.C; s.sdr = LDA; s.sdc = 1;
        s.M = c - off; s.N = ncols - off; s.K = cb; s.alpha = -1.0; s.beta = 1.0; s.mode = 0;
        s.sym_cols = struct_env ? c - off : 0;   // (the Schur complement of S: upper triangle only)
        gemm(h, s);
      }
    }
  } else
  for (int kb = 0; kb < c; kb += XK_CHOL_NB) {
    const int nb = std::min(XK_CHOL_NB, c - kb);
    const int rest = ncols - (kb + nb), mrem = c - kb - nb;
    XkCholStepArgs d{h->d_Maug, LDA, kb, nb, c, ncols, h->d_X, (rest + 15) / 16, h->d_status};
    hipLaunchKernelGGL(xk_chol_step, dim3(d.ncb * (1 + (mrem + 15) / 16)), dim3(64), 0, h->stream, d);
  }
  // P+ = sym(P - X^T X),  X = L^-1 W                   (I-KH)P, (P+P^T)/2
  if (u.cov_update) {
    memset(&g, 0, sizeof(g));
    g.A = h->d_X + c; g.sar = 1; g.sac = LDA;
    g.B = h->d_X + c; g.sbr = LDA; g.sbc = 1;
    g.D = u.Pin; g.sdr = 1; g.sdc = n;
    g.C = u.Pout; g.scr = 1; g.scc = n;
    g.M = n; g.N = n + 1; g.K = c; g.alpha = -1.0; g.beta = 1.0; g.mode = 2;
    g.sym_cols = struct_env ? n : 0;       // tiles below the diagonal: mirror images of the ones above
    // extra column: corr = X^T (L^-1 z') - corr_tot   (K z' - corr_tot, updater.cpp:126)
    g.xcol = 1; g.bx = h->d_X + c + n; g.sbx = LDA; g.ex = u.ct; g.cx = u.corr ? u.corr : h->d_corr; g.scx = 1;
    if (u.done_flag) { g.done_cnt = h->d_done_cnt; g.done_flag = u.done_flag; g.done_seq = u.done_seq; }
    gemm(h, g);
  } else {
    if (u.Pout != u.Pin) hipMemcpyAsync(u.Pout, u.Pin, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, h->stream);
    XkCorrArgs cr{h->d_X, LDA, c, n, c, c + n, u.ct, u.corr ? u.corr : h->d_corr};
    hipLaunchKernelGGL(xk_corr, dim3((n + 63) / 64), dim3(64), 0, h->stream, cr);
    if (u.done_flag) hipLaunchKernelGGL(xk_mark_done, dim3(1), dim3(1), 0, h->stream, u.done_flag, u.done_seq);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, XK_EDEVICE, "update launch", e);
  return XK_OK;
}

static int fetch_flags(xk_handle *h, int *inl, double *gam, int *inls, double *gams) {
  if (h->K > 0 && inl) HIPCHK(h, hipMemcpyAsync(inl, h->d_inl, sizeof(int) * h->K, hipMemcpyDeviceToHost, h->stream));
  if (h->K > 0 && gam) HIPCHK(h, hipMemcpyAsync(gam, h->d_gam, sizeof(double) * h->K, hipMemcpyDeviceToHost, h->stream));
  if (h->M > 0 && inls) HIPCHK(h, hipMemcpyAsync(inls, h->d_inl_s, sizeof(int) * h->M, hipMemcpyDeviceToHost, h->stream));
  if (h->M > 0 && gams) HIPCHK(h, hipMemcpyAsync(gams, h->d_gam_s, sizeof(double) * h->M, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// gate results of the last build -> the handle's pinned cache (asynchronous; valid after the next synchronisation)
static int cache_flags(xk_handle *h) {
  // MSCKF gate results: the per-feature kernel writes them into the pinned cache itself (XkFeatArgs::inlier_h / gamma_h);
  // without SLAM rows there is nothing to copy and nothing to wait for but the stream (five runtime calls less per frame)
  h->flags_direct = h->M == 0;
  if (!h->flags_direct) {
    HIPCHK(h, hipEventRecord(h->ev_flags, h->stream));               // the per-feature kernels have been queued
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_flags, 0));
    HIPCHK(h, hipMemcpyAsync(h->h_flag_i + h->Kmax, h->d_inl_s, sizeof(int) * h->M, hipMemcpyDeviceToHost, h->copy_stream));
    HIPCHK(h, hipMemcpyAsync(h->h_flag_d + h->Kmax, h->d_gam_s, sizeof(double) * h->M, hipMemcpyDeviceToHost, h->copy_stream));
    HIPCHK(h, hipEventRecord(h->ev_flags_done, h->copy_stream));
  }
  h->flags_cached = true;
  h->flags_after_seq = h->done_seq;
  return XK_OK;
}

// ---------------------------------------------------------------------------
// the pass every update entry queues, and its redo after a single launch that gave up
// ---------------------------------------------------------------------------
// The rows a pass works on.  REPLAY: see launch_build.  BUILT: launch_build has run already and the compression was left for now (the
// deferred stage of xk_build_compress_async): the pass starts behind the rows.
enum XkPassRows { XK_ROWS_BUILD, XK_ROWS_REPLAY, XK_ROWS_BUILT };

// One update queued from the staged inputs: the rows, the compression with the Kalman update offered to it (the single launch takes it
// along where it can), the separate Kalman launches where it did not.  Nothing here waits; the stage ends at "compressed", and who
// leaves the pass for xk_apply_update to collect says so itself (build_compress_update_pass).
// d_ct: correction_total on the device (NULL: zero).  cache: the gate flags go to the pinned cache (xk_fetch_flags).
// corr: where the correction goes -- NULL: h->d_corr, else pinned host memory (h->h_out).
// marker: (optional) the last launch writes a completion marker behind h->h_out; *marker = its sequence number (0 with XK_SPIN_DONE=0:
// wait for the stream).
// ev: (optional) five events recorded at the stage boundaries xk_bench_staged times -- before the rows, behind them, behind the first
// launch of the compression, behind the compression, behind the update.
static int queue_pass(xk_handle *h, double sigma_img, XkPassRows rows, const double *d_ct, int cov_update, bool cache, double *corr,
                      unsigned long long *marker = nullptr, hipEvent_t *ev = nullptr) {
  int rc;
  if (ev) HIPCHK(h, hipEventRecord(ev[0], h->stream));
  if (rows != XK_ROWS_BUILT && (rc = launch_build(h, sigma_img, rows == XK_ROWS_REPLAY)) != XK_OK) return rc;
  if (cache && (rc = cache_flags(h)) != XK_OK) return rc;
  if (ev) HIPCHK(h, hipEventRecord(ev[1], h->stream));
  UpdateSpec u = compressed_spec(h, d_ct, cov_update);
  u.corr = corr;
  if (marker) *marker = 0;
  if (marker && spin_done()) { u.done_flag = done_marker(h); *marker = u.done_seq = ++h->done_seq; }
  if ((rc = launch_compress(h, ev ? ev[2] : nullptr, &u)) != XK_OK) return rc;
  if (ev) HIPCHK(h, hipEventRecord(ev[3], h->stream));
  if (!h->last.fused && (rc = launch_update(h, u)) != XK_OK) return rc;   // (fused: the Kalman update was inside the compression's launch)
  if (ev) HIPCHK(h, hipEventRecord(ev[4], h->stream));
  return XK_OK;
}

// A single launch that gave up (XK_RETRY_CLASSIC) worked on nothing in place, but the multi-launch schedule that takes over does: the rows
// are built again -- the range / sun rows of the same update with them (replay) -- the gate flags cached again where the entry caches
// them, and the compression queued; the fast path has stepped aside, so the multi-launch schedule serves it.
// keep_rows: xk_apply_update redoing a compression that had been deferred.  The rows were linearised and gated at the prior, which the
// applyCI entries have replaced since, so they must NOT be rebuilt -- and they are still there: the single launch only read the tiles
// / factor records, and the multi-launch schedule, which works on the tiles in place, has not run.
static int redo_compress(xk_handle *h, bool cache, bool keep_rows = false) {
  int rc;
  if (keep_rows) h->upd.stage = XK_UPD_ROWS;      // (the give-up dropped the record)
  else {
    if ((rc = launch_build(h, h->sigma_img, true)) != XK_OK) return rc;
    if (cache && (rc = cache_flags(h)) != XK_OK) return rc;
  }
  return launch_compress(h);
}

// The one rule about retries: body(redo = false) may read its status words with allow_retry and end in XK_RETRY_CLASSIC -- the
// single-launch CAQR gave up, the prior is untouched -- and body(redo = true) then does the work again and may not: the multi-launch
// schedule cannot give up, so a give-up word met there is an error (give_up: XK_EDEVICE).
template <typename Body>
static int retry_once(Body body) {
  const int rc = body(false);
  return rc == XK_RETRY_CLASSIC ? body(true) : rc;
}

// correction_total of an update -> the device.  *d_ct = NULL where it is NULL or all zero (Updater::update starts every update from a zero
// correction_total: nothing to copy, and the Kalman launches skip the term), else h->d_ct behind a copy through the pinned ring.
static bool corr_total_zero(const xk_handle *h, const double *corr_total) {
  bool zero = true;
  if (corr_total)
    for (int i = 0; i < h->n && zero; ++i) zero = corr_total[i] == 0.0;
  return zero;
}
static int stage_corr_total(xk_handle *h, const double *corr_total, const double **d_ct) {
  *d_ct = nullptr;
  if (corr_total_zero(h, corr_total)) return XK_OK;
  double *st = (double *)stage_slot(h, sizeof(double) * h->n);
  if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
  memcpy(st, corr_total, sizeof(double) * h->n);
  HIPCHK(h, hipMemcpyAsync(h->d_ct, st, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
  *d_ct = h->d_ct;
  return XK_OK;
}

// ---------------------------------------------------------------------------
// public staged API
// ---------------------------------------------------------------------------
extern "C" int xk_msckf_build(xk_handle *h, double sigma_img, int *inlier_msckf, double *gamma_msckf,
                              int *inlier_slam, double *gamma_slam) {
  if (!h || !(sigma_img > 0.0)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = launch_build(h, sigma_img);
  if (rc != XK_OK) return rc;
  return fetch_flags(h, inlier_msckf, gamma_msckf, inlier_slam, gamma_slam);
}

extern "C" int xk_qr_compress(xk_handle *h, double *T_H, int ldt, double *z) {
  if (!h) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  h->want_full_T = true;                         // (this call hands out the reference's upper-triangular T_H: no split compression)
  const int rc = retry_once([&](bool redo) {
    const int rcq = redo ? redo_compress(h, false) : launch_compress(h);
    return rcq == XK_OK ? read_status(h, !redo) : rcq;
  });
  h->want_full_T = false;
  if (rc != XK_OK) return rc;
  if (T_H || z) {
    if (T_H && ldt < h->n) return XK_EINVAL;
    std::vector<double> R((size_t)h->C1 * h->C1P);
    HIPCHK(h, hipMemcpy(R.data(), h->d_R, sizeof(double) * R.size(), hipMemcpyDeviceToHost));
    if (T_H) {
      for (int j = 0; j < h->n; ++j)
        for (int i = 0; i < h->n; ++i) T_H[i + (size_t)j * ldt] = 0.0;
      // rows 0..na-1 of the triangle, placed at rows 0.. with the core columns zero
      for (int i = 0; i < h->na; ++i)
        for (int j = i; j < h->na; ++j) T_H[i + (size_t)(XK_CORE + j) * ldt] = R[(size_t)i * h->C1P + j];
    }
    if (z) {
      for (int i = 0; i < h->n; ++i) z[i] = 0.0;
      for (int i = 0; i < h->na; ++i) z[i] = R[(size_t)i * h->C1P + h->na];
    }
  }
  return XK_OK;
}

// xk_msckf_build + xk_qr_compress without a host synchronisation and without host outputs: the launches are queued behind
// whatever is already on the handle's stream (staging copies, covariance propagation, manage()) and xk_apply_update's
// one synchronisation covers them all.  The gate results come back with that synchronisation (xk_fetch_flags).
extern "C" int xk_build_compress_async(xk_handle *h, double sigma_img) {
  if (!h || !(sigma_img > 0.0)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = launch_build(h, sigma_img);
  if (rc != XK_OK) return rc;
  if ((rc = cache_flags(h)) != XK_OK) return rc;
  // Who calls this instead of xk_build_compress_update[_pass]_async has something between constructUpdate and applyUpdate that
  // rewrites the covariance (the applyCI entries of the MULTI_UAV order, updater.cpp:84-97).  [T_H | z] does not depend on the
  // covariance -- the gates have read the prior in the per-feature kernel above -- so where the single launch can take the Kalman
  // update along (narrow geometry, n <= 206) the compression is not queued now but by xk_apply_update, behind those entries, with
  // the Kalman role on the covariance they left: one launch there instead of one here and five there.
  const bool defer = h->opt_resident && h->persist_ok && kalman_rides(h) &&
                     h->K + h->K2 + h->M > 0 && h->plan < 2 &&   // (stacks that are not compressed at all: nothing to defer)
                     h->naux == 0;   // (range / sun rows: the update is not taken along by the launch anyway)
  if (defer) h->upd.stage = XK_UPD_ROWS_DEFERRED;
  else if ((rc = launch_compress(h)) != XK_OK) return rc;
  h->upd.unread = true;
  return XK_OK;
}

// The same with the Kalman update of Updater::applyUpdate(correction_total = 0, cov_update = true) queued as well -- inside the
// compression launch where the geometry allows it (xk_pipe_kalman), behind it otherwise.  xk_apply_update(h, NULL or zeros, 1, ..)
// then only waits for the result.  For callers that know at construction time that nothing comes between constructUpdate and
// applyUpdate (single agent, iekf_iter = 1: updater.cpp:99-110 with one pass) -- not the MULTI_UAV order, whose applyCI entries
// replace the covariance in between (updater.cpp:84-97).
static int build_compress_update_pass(xk_handle *h, double sigma_img, const double *corr_total, int cov_update) {
  if (!h || !(sigma_img > 0.0)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const double *dct = nullptr;
  int rc = stage_corr_total(h, corr_total, &dct);
  if (rc != XK_OK) return rc;
  unsigned long long seq;
  if ((rc = queue_pass(h, sigma_img, XK_ROWS_BUILD, dct, cov_update ? 1 : 0, true, h->h_out, &seq)) != XK_OK) return rc;
  // left for xk_apply_update, which must ask for the same
  XkPending &p = h->upd;
  p.stage = XK_UPD_QUEUED;
  p.unread = true;
  p.seq = seq;
  p.cov_update = cov_update ? 1 : 0;
  p.ct_zero = dct == nullptr;
  if (dct) memcpy(p.ct, corr_total, sizeof(double) * h->n);
  return XK_OK;
}
extern "C" int xk_build_compress_update_async(xk_handle *h, double sigma_img) { return build_compress_update_pass(h, sigma_img, nullptr, 1); }
extern "C" int xk_build_compress_update_pass_async(xk_handle *h, double sigma_img, const double *corr_total, int cov_update) {
  return build_compress_update_pass(h, sigma_img, corr_total, cov_update);
}

extern "C" int xk_fetch_flags(xk_handle *h, int *inlier_msckf, double *gamma_msckf, int *inlier_slam, double *gamma_slam) {
  if (!h) return XK_EINVAL;
  if (!h->flags_cached) return fail(h, XK_EINVAL, "xk_fetch_flags: no build since the inputs were staged");
  if (!h->flags_direct && hipEventQuery(h->ev_flags_done) != hipSuccess) {   // (normally long done: the copies ran beside the QR kernels)
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventSynchronize(h->ev_flags_done));
  }
  // the MSCKF results were written by the per-feature kernel: valid once the stream has passed it (after xk_apply_update
  // it has; otherwise this waits)
  // (a completion marker seen after the build was queued says the same without asking the runtime)
  if (h->K > 0 && !(h->done_seen > h->flags_after_seq) && hipStreamQuery(h->stream) != hipSuccess) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (inlier_msckf && h->K > 0) memcpy(inlier_msckf, h->h_flag_i, sizeof(int) * h->K);
  if (gamma_msckf && h->K > 0) memcpy(gamma_msckf, h->h_flag_d, sizeof(double) * h->K);
  if (inlier_slam && h->M > 0) memcpy(inlier_slam, h->h_flag_i + h->Kmax, sizeof(int) * h->M);
  if (gamma_slam && h->M > 0) memcpy(gamma_slam, h->h_flag_d + h->Kmax, sizeof(double) * h->M);
  return XK_OK;
}

// Gate result of the range row of the last build (range_update.cpp:246-262): *range_inlier 1 / 0, -1 if that build had no range row.
// Synchronises the stream.
extern "C" int xk_fetch_aux_flags(xk_handle *h, int *range_inlier, double *range_gamma) {
  if (!h) return XK_EINVAL;
  double f[2] = {0.0, 0.0};
  if (h->aux_mask & 1) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(f, h->d_aux + 3 * ((size_t)h->n + 1) + 3, sizeof(f), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (range_inlier) *range_inlier = (h->aux_mask & 1) ? (f[1] != 0.0 ? 1 : 0) : -1;
  if (range_gamma) *range_gamma = f[0];
  return XK_OK;
}

// The range / sun rows of the last build as built (h_lrf, h_sns, their residuals and r_diag entries, vio_updater.cpp:407-421), for a host
// that applies the dense system itself (xk_apply_update_dense).  H: rows x n, column-major, ldh >= 3 (any pointer may be NULL).
extern "C" int xk_aux_rows(xk_handle *h, double *H, int ldh, double *res, double *r_diag, int *rows) {
  if (!h) return XK_EINVAL;
  const int na = h->naux, n = h->n;
  if (H && ldh < 3) return XK_EINVAL;
  if (rows) *rows = na;
  if (na == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> b((size_t)3 * (n + 1) + 3);
  HIPCHK(h, hipMemcpyAsync(b.data(), h->d_aux, sizeof(double) * b.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int r = 0; r < na; ++r) {
    if (H)
      for (int c = 0; c < n; ++c) H[r + (size_t)c * ldh] = b[(size_t)r * (n + 1) + c];
    if (res) res[r] = b[(size_t)r * (n + 1) + n];
    if (r_diag) r_diag[r] = b[(size_t)3 * (n + 1) + r];
  }
  return XK_OK;
}

extern "C" int xk_apply_update(xk_handle *h, const double *corr_total, int cov_update, double *correction) {
  if (!h || !correction) return XK_EINVAL;
  // precondition: compressed, deferred or queued
  if (h->upd.stage < XK_UPD_ROWS_DEFERRED) return fail(h, XK_EINVAL, "xk_qr_compress has not run on the staged inputs");
  HIPCHK(h, hipSetDevice(h->device));
  // arguments first, before any state of the handle is touched: a mismatch with what xk_build_compress_update_async queued leaves the
  // queued update (posterior in d_Pout, marker, retry bookkeeping) exactly as it was -- the matching call can still collect it
  if (h->upd.stage == XK_UPD_QUEUED) {
    const XkPending &p = h->upd;
    const bool same = (cov_update ? 1 : 0) == p.cov_update &&
                      (p.ct_zero ? corr_total_zero(h, corr_total) : corr_total && memcmp(corr_total, p.ct, sizeof(double) * h->n) == 0);
    if (!same) return fail(h, XK_EINVAL, "xk_apply_update: not the correction_total / cov_update the queued pass was built with");
  }
  const double *dct = nullptr;
  int rc = stage_corr_total(h, corr_total, &dct);
  if (rc != XK_OK) return rc;
  // This call collects what is pending: the record keeps how far the device work has got (rows, or rows and [T_H | z]) and nothing that
  // a later call could collect a second time.
  const XkPending was = h->upd;
  const bool deferred = was.stage == XK_UPD_ROWS_DEFERRED, queued = was.stage == XK_UPD_QUEUED;
  const bool unread = was.unread || deferred;
  pending_drop(h);
  h->upd.stage = deferred ? XK_UPD_ROWS : XK_UPD_COMPRESSED;
  rc = retry_once([&](bool redo) -> int {
    int rc;
    // The kernels write the correction and (on failure) the status words into pinned host memory; the last workgroup of the
    // last launch then writes a sequence number next to them, which the host polls: the results are there ~5 us before the
    // runtime's completion signal says so (XK_SPIN_DONE=0: wait for that signal instead).  One wait per update, no copy.
    unsigned long long seq = 0;
    if (queued && !redo) seq = was.seq;                    // the update is already on the stream (xk_build_compress_update_async): only wait
    else if (deferred && !redo) {                          // the compression xk_build_compress_async left for now, Kalman role inside
      if ((rc = queue_pass(h, h->sigma_img, XK_ROWS_BUILT, dct, cov_update, false, h->h_out, &seq)) != XK_OK) return rc;
    } else {
      // (redo: the single-launch CAQR of the queued work gave up -- rows, compression and update again)
      if (redo && (rc = redo_compress(h, true, deferred)) != XK_OK) return rc;
      UpdateSpec u = compressed_spec(h, dct, cov_update);
      u.corr = h->h_out;
      if (spin_done()) { u.done_flag = done_marker(h); seq = u.done_seq = ++h->done_seq; }
      if ((rc = launch_update(h, u)) != XK_OK) return rc;
    }
    bool seen = false;
    if (seq) {
      // Acquire load: the correction and the status words read below are ordered after the marker.  The marker is the LAST
      // host-visible store of the update.  Separate Kalman launches: a system-scope RELEASE by the last workgroup of the last
      // kernel, after every workgroup of that kernel has been counted in (done_cnt).  Kalman role inside the single launch: the
      // correction and the status word are relaxed system-scope stores whose acknowledgement the writing wave waits for
      // (s_waitcnt vmcnt(0)) before it stores the marker, relaxed as well -- gfx950 behaviour, not a memory-model guarantee; the
      // -DXK_SYNC_STRICT=1 build stores that marker with a system-scope release (XK_MARKER_ORDER, xk_xcd_sync.hip.h).  In both forms
      // the marker covers ONLY the words in h_out: the posterior (d_Pout) may still be on its way out of the other waves when
      // the marker lands and is valid to later work through STREAM ORDER -- everything that reads it is queued on h->stream
      // behind this launch (the pointer swap below is host bookkeeping).  The kernels before it on the stream (whose failure
      // paths write the status words into the same pinned allocation) had completed, their stores released to system scope at
      // their kernel boundaries, before that kernel started: whatever they wrote is visible by the time the marker is.
      // (a single launch that gave up before its Kalman role got going -- placement census -- writes no marker: the status word
      //  ends the wait)
      seen = wait_marker(h, done_marker(h), seq);
      if (seen) h->done_seen = seq;
    }
    if (!seen) HIPCHK(h, hipStreamSynchronize(h->stream));
    stage_stream_idle(h);
    // (status words somebody has read already -- xk_qr_compress, settle_async -- cannot hold a give-up that is this update's to redo)
    return eval_status(h, h->d_status[0], h->d_status[1], unread && !redo);
  });
  if (rc != XK_OK) return rc;
  memcpy(correction, h->h_out, sizeof(double) * h->n);
  std::swap(h->d_P, h->d_Pout);  // posterior becomes the resident covariance
  pending_drop(h);
  return XK_OK;
}

extern "C" int xk_visual_update_staged(xk_handle *h, double sigma_img, double *correction, int *inlier_msckf,
                                       double *gamma_msckf, int *inlier_slam, double *gamma_slam) {
  if (!h || !correction || !(sigma_img > 0.0)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->K == 0 && h->K2 == 0 && h->M == 0 && !h->aux_staged) {  // h.size() == 0 -> no update (updater.cpp:106); MSCKF-SLAM rows count (vio_updater.cpp:413-419)
    for (int i = 0; i < h->n; ++i) correction[i] = 0.0;
    h->last.schedule = XK_SCHED_EMPTY;            // (xk_caqr_status: 4; staging dropped the pending update, or the compression it stands for was of this same empty stack: nothing else reads the record before the next one)
    return XK_OK;
  }
  const int rc = retry_once([&](bool redo) -> int {   // (the prior is untouched in d_P: the whole update is simply redone)
    int rc = queue_pass(h, sigma_img, redo ? XK_ROWS_REPLAY : XK_ROWS_BUILD, nullptr, 1, false, nullptr);
    if (rc != XK_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(correction, h->d_corr, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    rc = fetch_flags(h, inlier_msckf, gamma_msckf, inlier_slam, gamma_slam);
    return rc == XK_OK ? read_status(h, !redo) : rc;
  });
  if (rc != XK_OK) return rc;
  std::swap(h->d_P, h->d_Pout);
  pending_drop(h);
  return XK_OK;
}

extern "C" int xk_visual_update(xk_handle *h, const double *C_q_G, const double *G_p_C, int n_poses,
                                const int *trk_off, const double *obs_xy, int K, const double *feat,
                                const int *anchor_idxs, const int *track_sizes, const double *z_last, int M,
                                double *P, int ldp, int n, double sigma_img, double *correction,
                                int *inlier_msckf, double *gamma_msckf, int *inlier_slam, double *gamma_slam) {
  int rc;
  if ((rc = xk_stage_window(h, C_q_G, G_p_C, n_poses)) != XK_OK) return rc;
  if ((rc = xk_stage_tracks(h, trk_off, obs_xy, K)) != XK_OK) return rc;
  if ((rc = xk_stage_slam(h, feat, anchor_idxs, track_sizes, z_last, M)) != XK_OK) return rc;
  if ((rc = xk_stage_msckf_slam(h, nullptr, nullptr, 0)) != XK_OK) return rc;   // this entry point has no MSCKF-SLAM tracks
  if ((rc = xk_upload_P(h, P, ldp, n)) != XK_OK) return rc;
  if ((rc = xk_visual_update_staged(h, sigma_img, correction, inlier_msckf, gamma_msckf, inlier_slam,
                                    gamma_slam)) != XK_OK)
    return rc;
  return xk_download_P(h, P, ldp, n);
}

// ---------------------------------------------------------------------------
// dense (unfused) Kalman algebra
// ---------------------------------------------------------------------------
extern "C" int xk_apply_update_dense(xk_handle *h, double *P, int ldp, int n, const double *H, int ldh, int m,
                                     const double *res, const double *r_diag, double *correction_total,
                                     int cov_update, double *correction) {
  if (!h || !P || !H || !res || !r_diag || !correction || n != h->n || ldp < n || ldh < m || m <= 0) return XK_EINVAL;
  if (m > h->CM) return fail(h, XK_ECAPACITY, "m exceeds the dense workspace (n+1 rows); compress first");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy2DAsync(h->d_tmpP, sizeof(double) * n, P, sizeof(double) * ldp, sizeof(double) * n, n,
                             hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(h->d_tmpH, sizeof(double) * m, H, sizeof(double) * ldh, sizeof(double) * m, n,
                             hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_tmpz, res, sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_rdiag, r_diag, sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
  const double *dct = nullptr;
  if (correction_total) {
    HIPCHK(h, hipMemcpyAsync(h->d_ct, correction_total, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    dct = h->d_ct;
  }
  UpdateSpec u;
  memset(&u, 0, sizeof(u));
  u.T = h->d_tmpH; u.str = 1; u.stc = m;  // column-major m x n
  u.c = m; u.kdim = n; u.col0 = 0;
  u.z = h->d_tmpz; u.sz = 1; u.rdiag = h->d_rdiag;
  u.Pin = h->d_tmpP; u.Pout = h->d_Pout; u.ct = dct; u.cov_update = cov_update;
  int rc = launch_update(h, u);
  if (rc != XK_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(correction, h->d_corr, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(P, sizeof(double) * ldp, h->d_Pout, sizeof(double) * n, sizeof(double) * n, n,
                             hipMemcpyDeviceToHost, h->stream));
  rc = read_status(h);
  if (rc != XK_OK) return rc;
  if (correction_total)
    for (int i = 0; i < n; ++i) correction_total[i] += correction[i];  // updater.cpp:140
  return XK_OK;
}

// A build + compression queued by xk_build_compress_async whose single-launch CAQR gave up must be redone (multi-launch
// schedule) while the covariance it was linearised at is still the resident one: BEFORE a CI entry replaces it.  After this
// the compressed [T_H | z] is known to be good and xk_apply_update has nothing to retry.
static int settle_async(xk_handle *h) {
  if (!h->upd.unread) return XK_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  stage_stream_idle(h);
  int rc = eval_status(h, h->d_status[0], h->d_status[1], true);
  if (rc == XK_RETRY_CLASSIC) rc = redo_compress(h, true);   // (the multi-launch schedule: nothing left to read)
  if (rc == XK_OK) h->upd.unread = false;
  return rc;
}

// ---------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------
extern "C" int xk_bench_staged(xk_handle *h, double sigma_img, int warmup, int steps, xk_timing *out) {
  if (!h || !out || steps <= 0 || warmup < 0) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  memset(out, 0, sizeof(*out));
  const char *names[XK_NSTAGE] = {"xk_msckf_feature", "xk_slam_rows", "xk_caqr_panel0",
                                  "xk_caqr_rest",
                                  "xk_kalman_update", "(unused)"};
  for (int s = 0; s < XK_NSTAGE; ++s) snprintf(out->stage_name[s], sizeof(out->stage_name[s]), "%s", names[s]);
  double acc[XK_NSTAGE] = {0, 0, 0, 0, 0, 0}, tot = 0;
  const int rcm = retry_once([&](bool redo) -> int {   // (redo: the single-launch CAQR gave up somewhere -- measure the multi-launch schedule)
    for (int s = 0; s < XK_NSTAGE; ++s) acc[s] = 0;
    tot = 0;
    for (int it = 0; it < warmup + steps; ++it) {
      // (staged range / sun rows: in every step; fused: the Kalman update is inside stage 2's launch, stage 4 reads 0)
      const int rc = queue_pass(h, sigma_img, redo || it > 0 ? XK_ROWS_REPLAY : XK_ROWS_BUILD, nullptr, 1, false, nullptr, nullptr, h->ev);
      if (rc != XK_OK) return rc;
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (it >= warmup) {
        float ms;
        hipEventElapsedTime(&ms, h->ev[0], h->ev[1]); acc[0] += ms;
        hipEventElapsedTime(&ms, h->ev[1], h->ev[2]); acc[2] += ms;
        hipEventElapsedTime(&ms, h->ev[2], h->ev[3]); acc[3] += ms;
        hipEventElapsedTime(&ms, h->ev[3], h->ev[4]); acc[4] += ms;
        hipEventElapsedTime(&ms, h->ev[0], h->ev[4]); tot += ms;
      }
    }
    return read_status(h, !redo);
  });
  if (rcm != XK_OK) return rcm;
  for (int s = 0; s < XK_NSTAGE; ++s) out->stage_ms[s] = (float)(acc[s] / steps);
  out->total_ms = (float)(tot / steps);
  out->stage_launches[0] = (h->K > 0) + (h->M > 0);
  out->stage_launches[2] = 1;
  out->stage_launches[3] = outcome_single(h->last) ? 0 : h->last.launches;   // (the single launch IS stage 2's one launch)
  const int nblk = (h->na + XK_CHOL_NB - 1) / XK_CHOL_NB;
  out->stage_launches[4] = h->last.fused ? 0 : 4 + 3 * nblk;
  out->n = h->n; out->c1 = h->C1; out->k_tracks = h->K; out->n_leaf = h->last.leaves; out->n_levels = h->last.launches;
  // stacked rows actually folded (inlier rows)
  {
    const int slam_tiles = (2 * h->M + h->DB - 1) / h->DB;
    std::vector<int> tr(h->K + h->K2 + slam_tiles);
    HIPCHK(h, hipMemcpy(tr.data(), h->d_tile_rows, sizeof(int) * tr.size(), hipMemcpyDeviceToHost));
    int rows = 0;
    for (int v : tr) rows += v;
    out->rows_stacked = rows;
  }
  // leave the posterior of the last step in d_Pout; the staged prior stays in d_P
  return XK_OK;
}

extern "C" int xk_run_steps(xk_handle *h, double sigma_img, int steps) {
  if (!h || steps < 0 || !(sigma_img > 0.0)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
#ifdef XK_LAB
  static const int use_graph = env_int("XK_GRAPH", 0);
  if (use_graph && steps > 1) {
    // experiment: the 30 launches of one update captured once and replayed
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    int rc = queue_pass(h, sigma_img, XK_ROWS_BUILD, nullptr, 1, false, nullptr);
    hipError_t e = hipStreamEndCapture(h->stream, &g);
    if (rc != XK_OK) return rc;
    if (e != hipSuccess) return fail(h, XK_EDEVICE, "graph capture", e);
    HIPCHK(h, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    for (int it = 0; it < steps; ++it) HIPCHK(h, hipGraphLaunch(ge, h->stream));
    rc = read_status(h);
    hipGraphExecDestroy(ge);
    hipGraphDestroy(g);
    return rc;
  }
#endif
  // (every step recomputes the same update from the resident prior, so a single-launch CAQR that gave up -- e.g. two
  //  processes sharing one GPU, each with a grid that wants every CU -- costs one more pass with the multi-launch schedule)
  return retry_once([&](bool redo) {
    for (int it = 0; it < steps; ++it) {
      const int rc = queue_pass(h, sigma_img, redo || it > 0 ? XK_ROWS_REPLAY : XK_ROWS_BUILD, nullptr, 1, false, nullptr);   // (staged range / sun rows: in every step)
      if (rc != XK_OK) return rc;
    }
    return read_status(h, !redo);
  });
}
