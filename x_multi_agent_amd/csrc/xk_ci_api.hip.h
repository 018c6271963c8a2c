// xk_ci_api.hip.h -- host side of the covariance-intersection entries: the fuse / match / track entries of the reference's CI
// (ci.cpp, multi_slam_update.cpp, msckf_update.cpp:96-279) with fixed or searched weights, applyCI on a dense H, the
// device-resident CI round and the inter-agent payload.  Part of xk_api.hip's translation unit, included behind launch_update,
// the staging helpers and settle_async.
#pragma once

// ---------------------------------------------------------------------------
// covariance intersection: fixed weights, or searched ones (option "ci_weight_search", xk_ciw.hip.h)
// ---------------------------------------------------------------------------
// a rows x cols column-major matrix between host and device (leading dimensions ldd / lds), on the engine's stream
static hipError_t copy_matrix(xk_handle *h, double *dst, int ldd, const double *src, int lds, int rows, int cols, hipMemcpyKind kind) {
  return hipMemcpy2DAsync(dst, sizeof(double) * ldd, src, sizeof(double) * lds, sizeof(double) * rows, cols, kind, h->stream);
}

// 0: a fixed weight; 1: -1 <= w < 0 with the search switched on (ci.cpp:65-73,105-119); -1: what ci.cpp:59-62,98-101 throw on,
// and every negative weight while the search is off
static int check_w(const xk_handle *h, double w) {
  if (w > 1.0 || w == 0 || w < -1) return -1;
  if (w < 0.0) return h->opt_ci_search ? 1 : -1;
  return 0;
}

// the entry's device-side weights, the start point of a search, its two result words, and per agent M_i and H_i P_i H_i^T
static double *ciw_M(xk_handle *h, int i) { return h->d_ciw + 24 + (size_t)i * 576; }
static double *ciw_T(xk_handle *h, int i) { return h->d_ciw + 24 + (size_t)(XK_CIW_MAXK1 + i) * 576; }

static void ciw_set(xk_handle *h, double *slot, const double *v, int k1) {
  XkCiwSetArgs s;
  s.w = slot;
  for (int i = 0; i < XK_CIW_MAXK1; ++i) s.v[i] = i < k1 ? v[i] : 0.0;
  hipLaunchKernelGGL(xk_ciw_set, dim3(1), dim3(64), 0, h->stream, s);
}

// the entry's two fixed weights: own, other (the multi-agent form keeps ONE weight for all the other agents, in slot 1)
static void ciw_set_fixed(xk_handle *h, double w_own, double w_other) {
  const double v[2] = {w_own, w_other};
  ciw_set(h, h->d_ciw, v, 2);
}

// S (m x m in Sd) (+)= T / w_i with the weights of the entry's device slots (xk_ciw_sum)
static void ciw_sum(xk_handle *h, const double *T, double *Sd, int m, int i, bool pair, bool first, bool add_diag, double diag,
                    double *d_w_result) {
  XkCiwSumArgs s{T, Sd, m, first ? 1 : 0, i, pair ? 1 : 0, add_diag ? 1 : 0, diag, h->d_ciw, d_w_result};
  hipLaunchKernelGGL(xk_ciw_sum, dim3((m * m + 255) / 256), dim3(256), 0, h->stream, s);
}

// C (M x N) = A (M x K) B (K x N) for xk_gemm_f64, every operand by its row / column strides; alpha 1, beta 0, D = C
static XkGemmArgs gemm_args(const double *A, long sar, long sac, const double *B, long sbr, long sbc, double *C, long scr, long scc,
                            int M, int N, int K) {
  XkGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.sar = sar; g.sac = sac;
  g.B = B; g.sbr = sbr; g.sbc = sbc;
  g.C = C; g.scr = scr; g.scc = scc; g.D = g.C; g.sdr = scr; g.sdc = scc;
  g.M = M; g.N = N; g.K = K; g.alpha = 1.0; g.beta = 0.0;
  return g;
}

// H P H^T by two GEMMs: W = Hd Pd (Hd m x nn column-major, W m x nn row-major in d_Maug) ...
static void hp_product(xk_handle *h, const double *Hd, const double *Pd, int m, int nn) { gemm(h, gemm_args(Hd, 1, m, Pd, 1, nn, h->d_Maug, nn, 1, m, nn, nn)); }
// ... and T (m x m, ld m) = W Hd^T (B[k][j] = H[j][k]); the caller may change beta / mode / diag_scalar before it launches
static XkGemmArgs wht_args(xk_handle *h, const double *Hd, int m, int nn, double *T) { return gemm_args(h->d_Maug, nn, 1, Hd, m, 1, T, 1, m, m, m, nn); }
// T (device, m x m, ld m) = Hd (m x nn col-major) * Pd (nn x nn) * Hd^T
static void hpht(xk_handle *h, const double *Hd, const double *Pd, int m, int nn, double *T) {
  hp_product(h, Hd, Pd, m, nn);
  gemm(h, wht_args(h, Hd, m, nn, T));
}

// Information projection M = Hd Pd^-1 Hd^T (m x m, ld m) with the Kalman stage's factorisation: the system is [P | H^T],
// xk_chol_whole per 192-row slab with the Schur-complement GEMM between slabs (launch_update), X = L^-1 H^T, M = X^T X.
// ONE factorisation of Pd serves all m right-hand sides.  A pivot that is not positive sets the handle's status word.
static int ci_info(xk_handle *h, const double *Hd, const double *Pd, int m, int nn, double *Mout) {
  const int LDA = h->LDA, c = nn, ncols = nn + m;
  if (nn > h->CM || ncols > LDA) return fail(h, XK_ECAPACITY, "CI weight search: covariance exceeds the workspace");
  XkCopyArgs cp{Pd, h->d_Maug, nn, nn, 1, (long)nn, (long)LDA, 1};
  hipLaunchKernelGGL(xk_copy2d, dim3((nn * nn + 255) / 256), dim3(256), 0, h->stream, cp);
  XkCopyArgs ch{Hd, h->d_Maug + nn, nn, m, (long)m, 1, (long)LDA, 1};        // row r of the right-hand sides = column r of H
  hipLaunchKernelGGL(xk_copy2d, dim3((nn * m + 255) / 256), dim3(256), 0, h->stream, ch);
  const int B = 16 * XK_CHOLW_MAXB;
  for (int off = 0; off < c;) {
    const int cb = std::min(B, c - off);
    XkCholWholeArgs d;
    d.Maug = h->d_Maug + (size_t)off * LDA + off; d.ld = LDA; d.c = cb; d.ncols = ncols - off;
    d.X = h->d_X + (size_t)off * LDA + off; d.status = h->d_status;
#ifdef XK_CHOLW_PROBE
    d.dbg = nullptr;
#endif
    xk_cholw_table((cb + 15) / 16, d.tab);
    hipLaunchKernelGGL(xk_chol_whole, dim3((ncols - off - cb + 15) / 16), dim3(64 * XK_CHOLW_WAVES), 0, h->stream, d);
    off += cb;
    if (off < c) {
      const double *Xs = h->d_X + (size_t)(off - cb) * LDA + off;
      XkGemmArgs s = gemm_args(Xs, 1, LDA, Xs, LDA, 1, h->d_Maug + (size_t)off * LDA + off, LDA, 1, c - off, ncols - off, cb);
      s.alpha = -1.0; s.beta = 1.0;
      s.sym_cols = c - off;
      gemm(h, s);
    }
  }
  gemm(h, gemm_args(h->d_X + nn, 1, LDA, h->d_X + nn, LDA, 1, Mout, 1, m, m, m, nn));   // A[i][k] = X[k][nn + i], B[k][j] = X[k][nn + j]
  return XK_OK;
}

// after the stream has been synchronised: did a factorisation of ci_info meet a pivot that is not positive?
static int ciw_chol_status(xk_handle *h) {
  if (h->d_status[0] == 0) return XK_OK;
  h->d_status[0] = 0;
  return fail(h, XK_ESINGULAR, "CI weight search: a covariance is not positive definite");
}

// queue the search over the k1 matrices in ciw_M (stride mstride); start = null: from the uniform point
static void ciw_solve(xk_handle *h, int m, int k1, int mstride, const double *start) {
  if (start) ciw_set(h, h->d_ciw + 8, start, k1);
  XkCiwArgs a{ciw_M(h, 0), 0, mstride, m, k1, start ? h->d_ciw + 8 : nullptr, h->d_ciw, (int *)(h->d_ciw + 16), nullptr};
  hipLaunchKernelGGL(xk_ci_weights, dim3(1), dim3(XK_CIW_THREADS), 0, h->stream, a);
}

// the solver's failure word is set: it ran out of Newton steps, or met a sum that is not positive definite
static int ciw_search_failed(xk_handle *h, int iters) {
  return fail(h, XK_ESINGULAR, iters >= XK_CIW_MAXIT ? "CI weight search: no convergence within 50 Newton steps"
                                                      : "CI weight search: sum w_i M_i is not positive definite");
}

// fetch the searched weights (synchronises), check both failure words, remember them for xk_ci_last_weights
static int ciw_fetch(xk_handle *h, int k1, double *w) {
  double buf[17];
  HIPCHK(h, hipMemcpyAsync(buf, h->d_ciw, sizeof(buf), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (int rc = ciw_chol_status(h)) return rc;
  int info[2];
  memcpy(info, buf + 16, sizeof(info));
  if (info[1] != 0) return ciw_search_failed(h, info[0]);
  for (int i = 0; i < 8; ++i) h->ci_last_w[i] = i < k1 ? buf[i] : 0.0;
  h->ci_last_k1 = k1;
  h->ci_last_iters = info[0];
  if (w) memcpy(w, buf, sizeof(double) * k1);
  return XK_OK;
}

// start points of the two forms.  The reference's own (ci.cpp:66-67,109-110) are infeasible for k agents resp. for w = -1 and make
// NLopt give up; these are feasible, and the result does not depend on them.
static void ciw_start_pair(double w, double *st) {
  st[1] = std::min(std::max(-w, XK_CIW_LB), 1.0 - XK_CIW_LB);
  st[0] = 1.0 - st[1];
}
static const double *ciw_start_multi(double w, int k, double *st) {
  const double wo = -w, w0 = 1.0 - k * wo;
  if (!(wo >= XK_CIW_LB) || !(w0 >= XK_CIW_LB)) return nullptr;      // uniform
  st[0] = w0;
  for (int i = 1; i <= k; ++i) st[i] = wo;
  return st;
}

// One agent's operands of a fuse entry, on the host: P_i (n x n column-major, leading dimension ldp) and H_i (m x n, ldh).
struct CiFuseAgent {
  const double *P;
  int ldp, n;
  const double *H;
  int ldh;
};

// S = sum_i H_i P_i H_i^T / w_i over k1 agents, to the host (m x m, lds).  pair: the pairwise form of xk_ciw_sum (own weight
// 1 - w[1]).  Fixed weights (srch = 0) are in the entry's device slots already (ciw_set by the caller) and every term joins the sum
// at once; the multi-agent form keeps ONE weight for all the other agents, in slot 1.  Searched: H_i P_i H_i^T and M_i are kept
// until the search from `start` (null: the uniform point) has run; w receives its k1 weights.
static int fuse_ci(xk_handle *h, const CiFuseAgent *ag, int k1, int m, bool pair, int srch, const double *start, double *w, double *S,
                   int lds) {
  for (int i = 0; i < k1; ++i) {
    const CiFuseAgent &a = ag[i];
    if (i) HIPCHK(h, hipStreamSynchronize(h->stream));   // d_tmpP and d_tmpH are used again
    HIPCHK(h, copy_matrix(h, h->d_tmpP, a.n, a.P, a.ldp, a.n, a.n, hipMemcpyHostToDevice));
    HIPCHK(h, copy_matrix(h, h->d_tmpH, m, a.H, a.ldh, m, a.n, hipMemcpyHostToDevice));
    double *T = srch ? ciw_T(h, i) : h->d_X;
    hpht(h, h->d_tmpH, h->d_tmpP, m, a.n, T);
    if (!srch) ciw_sum(h, T, h->d_tmpS, m, (pair || i == 0) ? i : 1, pair, i == 0, false, 0.0, nullptr);
    else if (int rc = ci_info(h, h->d_tmpH, h->d_tmpP, m, a.n, ciw_M(h, i))) return rc;
  }
  if (srch) {
    ciw_solve(h, m, k1, 576, start);
    if (int rc = ciw_fetch(h, k1, w)) return rc;
    for (int i = 0; i < k1; ++i) ciw_sum(h, ciw_T(h, i), h->d_tmpS, m, i, pair, i == 0, false, 0.0, nullptr);
  }
  HIPCHK(h, copy_matrix(h, S, lds, h->d_tmpS, m, m, m, hipMemcpyDeviceToHost));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

extern "C" int xk_fuse_ci_msckf(xk_handle *h, const double *P, int ldp, int n, const double *H, int ldh, int m,
                                int k, const double *const *Ps, const int *ns, const double *const *Hs,
                                double w_other, double *S, int lds, double *w_result) {
  if (!h || !P || !H || !S || !w_result || k < 0 || m <= 0 || ldp < n || ldh < m || lds < m) return XK_EINVAL;
  const int srch = check_w(h, w_other);
  if (srch < 0) return fail(h, XK_EINVAL, "The CI weights must be lower than 1.0 and larger 0.0");
  if (n > h->n || m > h->CM) return fail(h, XK_ECAPACITY, "fuse_ci dims exceed workspace");
  if (srch && k < 1) return fail(h, XK_EINVAL, "CI weight search: no other agent");
  if (srch && (m > XK_CIW_MAXM || k + 1 > XK_CIW_MAXK1)) return fail(h, XK_ECAPACITY, "CI weight search: at most 21 rows and 7 other agents");
  std::vector<CiFuseAgent> ag(k + 1);
  ag[0] = {P, ldp, n, H, ldh};
  for (int i = 1; i <= k; ++i) {                                       // (the other agents' arrays are contiguous)
    if (ns[i - 1] > h->n) return fail(h, XK_ECAPACITY, "other agent's state larger than workspace");
    ag[i] = {Ps[i - 1], ns[i - 1], ns[i - 1], Hs[i - 1], m};
  }
  HIPCHK(h, hipSetDevice(h->device));
  const double w0 = 1.0 - (double)k * w_other;
  if (!srch) ciw_set_fixed(h, w0, w_other);
  double st[XK_CIW_MAXK1], w[XK_CIW_MAXK1];
  if (int rc = fuse_ci(h, ag.data(), k + 1, m, false, srch, srch ? ciw_start_multi(w_other, k, st) : nullptr, w, S, lds)) return rc;
  *w_result = srch ? 1.0 / w[0] : 1.0 / w0;                            // ci.cpp:78-90, with the searched w_0
  return XK_OK;
}

extern "C" int xk_fuse_ci_slam(xk_handle *h, const double *Pa, int lda, int na, const double *Ha, int ldha,
                               const double *Pb, int ldb, int nb, const double *Hb, int ldhb, int m,
                               double w_other, double *S, int lds, double *w_result) {
  if (!h || !Pa || !Ha || !Pb || !Hb || !S || !w_result || m <= 0 || lda < na || ldb < nb || ldha < m || ldhb < m ||
      lds < m)
    return XK_EINVAL;
  const int srch = check_w(h, w_other);
  if (srch < 0) return fail(h, XK_EINVAL, "The CI weights must be lower than 1.0 and larger than 0.0");
  if (na > h->n || nb > h->n || m > h->CM) return fail(h, XK_ECAPACITY, "fuse_ci dims exceed workspace");
  if (srch && m > XK_CIW_MAXM) return fail(h, XK_ECAPACITY, "CI weight search: at most 21 rows");
  HIPCHK(h, hipSetDevice(h->device));
  double st[2], w[2];
  if (!srch) ciw_set_fixed(h, 1.0 - w_other, w_other);
  else ciw_start_pair(w_other, st);
  const CiFuseAgent ag[2] = {{Pa, lda, na, Ha, ldha}, {Pb, ldb, nb, Hb, ldhb}};
  if (int rc = fuse_ci(h, ag, 2, m, true, srch, st, w, S, lds)) return rc;
  *w_result = 1.0 / (1.0 - (srch ? w[1] : w_other));                   // ci.cpp:117-122, with the searched w_b
  return XK_OK;
}

extern "C" int xk_multi_slam_match(xk_handle *h, const double *C_q_G, const double *G_p_C, int n_poses,
                                   const double *feat, int anchor_idx, int feature_id, const double *P, int ldp,
                                   int n, int n_poses_max, const double *o_C_q_G, const double *o_G_p_C,
                                   int o_n_poses, const double *o_feat, int o_anchor_idx, int o_feature_id,
                                   const double *o_P, int ldop, int no, int o_n_poses_max, double sigma_landmark,
                                   double ci_slam_w, int *inlier, double *gamma, double *H, int ldh, double *res,
                                   double *S, double *P_j, int ldpj) {
  if (!h || !C_q_G || !G_p_C || !feat || !P || !o_C_q_G || !o_G_p_C || !o_feat || !o_P || !inlier || !gamma || !H ||
      !res || !S || !P_j)
    return XK_EINVAL;
  if (anchor_idx < 0) return fail(h, XK_EINVAL, "anchor_idx < 0");       // throws, multi_slam_update.cpp:83-85
  if (n != h->n || ldp < n || ldop < no || ldh < 3 || ldpj < n) return XK_EINVAL;
  const int Mf = (n - XK_CORE - 6 * n_poses_max) / 3, oMf = (no - XK_CORE - 6 * o_n_poses_max) / 3;
  if (feature_id < 0 || feature_id >= Mf || o_feature_id < 0 || o_feature_id >= oMf || anchor_idx >= n_poses ||
      o_anchor_idx < 0 || o_anchor_idx >= o_n_poses)
    return XK_EINVAL;
  if (feat[3 * feature_id + 2] == 0) return fail(h, XK_EINVAL, "rho = 0");  // throws, :86-88
  const int srch = check_w(h, ci_slam_w);
  if (srch < 0) return fail(h, XK_EINVAL, "The CI weights must be lower than 1.0 and larger than 0.0");
  if (no > h->n || n_poses > h->N || o_n_poses > h->N) return fail(h, XK_ECAPACITY, "match dims exceed workspace");
  HIPCHK(h, hipSetDevice(h->device));
  // scratch layout in d_ci
  double *d = h->d_ci;
  double *dq = d, *dp = dq + 4 * h->N, *df = dp + 3 * h->N, *doq = df + 3 * (Mf > 0 ? Mf : 1);
  double *dop = doq + 4 * h->N, *dof = dop + 3 * h->N, *dH = dof + 3 * (oMf > 0 ? oMf : 1);
  double *dout = dH + 3 * (size_t)n, *dcols_f = dout + 16, *doH = dcols_f + 2;
  int *dcols = (int *)dcols_f;
  double *doP = h->d_ci + 64 * (size_t)h->n + 1024;   // (the lists above end long before: < 11 n + 64 doubles)
  HIPCHK(h, hipMemcpyAsync(dq, C_q_G, sizeof(double) * 4 * n_poses, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dp, G_p_C, sizeof(double) * 3 * n_poses, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(df, feat, sizeof(double) * 3 * Mf, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(doq, o_C_q_G, sizeof(double) * 4 * o_n_poses, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dop, o_G_p_C, sizeof(double) * 3 * o_n_poses, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dof, o_feat, sizeof(double) * 3 * oMf, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, copy_matrix(h, h->d_tmpP, n, P, ldp, n, n, hipMemcpyHostToDevice));
  HIPCHK(h, copy_matrix(h, doP, no, o_P, ldop, no, no, hipMemcpyHostToDevice));
  XkSlamMatchArgs a;
  a.q = dq; a.p = dp; a.feat = df; a.P = h->d_tmpP; a.anchor = anchor_idx; a.fid = feature_id; a.n = n; a.npm = n_poses_max;
  a.oq = doq; a.op = dop; a.ofeat = dof; a.oP = doP; a.oanchor = o_anchor_idx; a.ofid = o_feature_id; a.no = no;
  a.onpm = o_n_poses_max;
  a.var_l = sigma_landmark * sigma_landmark; a.w = h->d_ciw; a.chi = XK_CHI2_090[3];
  a.H = dH; a.out = dout; a.cols = dcols; a.oH = nullptr; a.gate_only = 0;
  if (!srch) ciw_set_fixed(h, 1.0 - ci_slam_w, ci_slam_w);
  else {
    // the Jacobians and the gate first (neither depends on the weights, multi_slam_update.cpp:216-220 precedes :222), then the two
    // information projections and the search; the launch below reads the searched w_b
    a.oH = doH; a.gate_only = 1;
    hipLaunchKernelGGL(xk_slam_match, dim3(1), dim3(64), 0, h->stream, a);
    a.oH = nullptr; a.gate_only = 0;
    int rc = ci_info(h, dH, h->d_tmpP, 3, n, ciw_M(h, 0));
    if (rc == XK_OK) rc = ci_info(h, doH, doP, 3, no, ciw_M(h, 1));
    if (rc != XK_OK) return rc;
    double st[2];
    ciw_start_pair(ci_slam_w, st);
    ciw_solve(h, 3, 2, 576, st);
    if ((rc = ciw_fetch(h, 2, nullptr)) != XK_OK) return rc;
  }
  hipLaunchKernelGGL(xk_slam_match, dim3(1), dim3(64), 0, h->stream, a);
  XkScaleArgs sc{h->d_tmpP, h->d_Pout, n, 3, dcols, dout + 14};
  hipLaunchKernelGGL(xk_scale_blocks, dim3(((size_t)n * n + 255) / 256), dim3(256), 0, h->stream, sc);
  double hout[16];
  HIPCHK(h, hipMemcpyAsync(hout, dout, sizeof(double) * 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, copy_matrix(h, H, ldh, dH, 3, 3, n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 3; ++i) res[i] = hout[i];
  *gamma = hout[12];
  *inlier = hout[13] != 0.0;
  if (*inlier) {
    for (int i = 0; i < 9; ++i) S[i] = hout[3 + i];
    HIPCHK(h, copy_matrix(h, P_j, ldpj, h->d_Pout, n, n, n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return XK_OK;
}

// ---------------------------------------------------------------------------
// MSCKF-MSCKF CI block (msckf_update.cpp:96-279) for one track
// ---------------------------------------------------------------------------
// The joint gate's threshold chi2(0.95, dof) (:245-247), compared on the host in both routes: from the table, and past its 512
// degrees of freedom (eight agents with windows of 33 and more) from the quantile function (as slam_gate_threshold at 0.9).
static double ci_gate_threshold(int dof) { return dof < XK_CHI2_LEN ? XK_CHI2_095[dof] : xk_chi2_quantile_host(0.95, dof); }

extern "C" int xk_msckf_ci_track(xk_handle *h, const double *obs, int L, const double *C_q_G, const double *G_p_C,
                                 int n_poses, const double *P, int ldp, int n, int n_poses_max, double sigma_img,
                                 int k, const double *const *m_obs, const int *m_L, const double *const *m_q,
                                 const double *const *m_p, const int *m_nposes, const int *m_nposes_max,
                                 const double *const *m_P, const int *m_n, double ci_msckf_w, int *self_inlier,
                                 double *self_gamma, int *has_ci, double *ci_gamma, double *H, int ldh, double *res, double *S,
                                 int lds, double *P_j, int ldpj) {
  if (!h || !obs || !C_q_G || !G_p_C || !P || !self_inlier || !self_gamma || !has_ci || k < 0) return XK_EINVAL;
  if (k > XK_CI_MAXK) return fail(h, XK_ECAPACITY, "more than 7 matched agents");
  if (n != h->n || ldp < n || L < 2 || L > n_poses || n_poses > h->N || n_poses_max != h->N) return XK_EINVAL;
  if (k > 0 && (!m_obs || !m_L || !m_q || !m_p || !m_nposes || !m_nposes_max || !m_P || !m_n || !H || !res || !S || !P_j || !ci_gamma ||
                ldh < 3 * k || lds < 3 * k || ldpj < n))
    return XK_EINVAL;
  const int srch = k > 0 ? check_w(h, ci_msckf_w) : 0;
  if (srch < 0) return fail(h, XK_EINVAL, "The CI weights must be lower than 1.0 and larger 0.0");
  int Ltot = L, nmax = n;
  for (int i = 0; i < k; ++i) {
    // a matched agent's lists hold its VALID poses; its covariance is laid out for its own window size (include/xk.h)
    if (m_L[i] < 2 || m_L[i] > m_nposes[i] || m_nposes[i] > m_nposes_max[i] || m_nposes_max[i] > 64 ||
        m_n[i] < XK_CORE + 6 * m_nposes_max[i])
      return XK_EINVAL;
    Ltot += m_L[i];
    nmax = std::max(nmax, m_n[i]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  *has_ci = 0;
  const int m = 3 * k, k1 = k + 1;
  // workspace (lazily sized): concatenated lists, per-agent window/obs/P, up rows, H blocks, S buffers
  const size_t upsz = 3 * (size_t)nmax + 16;
  const size_t need = 9 * (size_t)Ltot + 7 * 64 + 2 * 64 + (size_t)nmax * nmax + k1 * upsz + (size_t)std::max(m, 1) * k1 * nmax +
                      4 * 24 * 24 + 1024;
  double *ws = nullptr;
  HIPCHK(h, hipMalloc((void **)&ws, sizeof(double) * need));
  struct Guard { double *p; ~Guard() { if (p) hipFree(p); } } guard{ws};
  double *dq = ws, *dp = dq + 4 * (size_t)Ltot, *dobs = dp + 3 * (size_t)Ltot;
  double *aq = dobs + 2 * (size_t)Ltot, *ap = aq + 4 * 64, *aobs = ap + 3 * 64;   // one agent's window + track
  double *aP = aobs + 2 * 64, *up = aP + (size_t)nmax * nmax, *Hs = up + k1 * upsz;
  double *S1 = Hs + (size_t)std::max(m, 1) * k1 * nmax, *S2 = S1 + 24 * 24, *dres = S2 + 24 * 24, *dgpf = dres + 24;
  double *dscal = dgpf + 8;  // [0] ci gamma, [1] w_result
  int *dint = (int *)(dscal + 8);  // [0] gn iters, [1] inlier, [2] tile rows, [3..] block columns
  // concatenated lists: matched agents first, self last (:113-149)
  size_t at = 0;
  for (int i = 0; i < k; ++i) {
    HIPCHK(h, hipMemcpyAsync(dq + 4 * at, m_q[i] + 4 * (size_t)(m_nposes[i] - m_L[i]), sizeof(double) * 4 * m_L[i], hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dp + 3 * at, m_p[i] + 3 * (size_t)(m_nposes[i] - m_L[i]), sizeof(double) * 3 * m_L[i], hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dobs + 2 * at, m_obs[i], sizeof(double) * 2 * m_L[i], hipMemcpyHostToDevice, h->stream));
    at += m_L[i];
  }
  HIPCHK(h, hipMemcpyAsync(dq + 4 * at, C_q_G + 4 * (size_t)(n_poses - L), sizeof(double) * 4 * L, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dp + 3 * at, G_p_C + 3 * (size_t)(n_poses - L), sizeof(double) * 3 * L, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dobs + 2 * at, obs, sizeof(double) * 2 * L, hipMemcpyHostToDevice, h->stream));
  XkTriMultiArgs ta{dq, dp, dobs, Ltot, dgpf, dint, nullptr, 0};
  hipLaunchKernelGGL(xk_triangulate_multi, dim3(1), dim3(64), 0, h->stream, ta);
  // per-agent column-space rows (self first = row block 0, then the matched agents, :168-204)
  for (int i = 0; i < k1; ++i) {
    const bool self = (i == 0);
    const double *hq = self ? C_q_G : m_q[i - 1], *hp = self ? G_p_C : m_p[i - 1], *hobs = self ? obs : m_obs[i - 1];
    const double *hP = self ? P : m_P[i - 1];
    const int np_i = self ? n_poses : m_nposes[i - 1], L_i = self ? L : m_L[i - 1], n_i = self ? n : m_n[i - 1];
    const int ld_i = self ? ldp : n_i, npm_i = self ? n_poses_max : m_nposes_max[i - 1];
    HIPCHK(h, hipStreamSynchronize(h->stream));  // scratch reuse across agents
    HIPCHK(h, hipMemcpyAsync(aq, hq, sizeof(double) * 4 * np_i, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ap, hp, sizeof(double) * 3 * np_i, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(aobs, hobs, sizeof(double) * 2 * L_i, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, copy_matrix(h, aP, n_i, hP, ld_i, n_i, n_i, hipMemcpyHostToDevice));
    const int toff[2] = {0, L_i};
    HIPCHK(h, hipMemcpyAsync(dint + 8, toff, sizeof(int) * 2, hipMemcpyHostToDevice, h->stream));
    XkFeatArgs a;
    memset(&a, 0, sizeof(a));
    a.q = aq; a.p = ap; a.n_poses = np_i; a.n_poses_max = npm_i; a.trk_off = dint + 8; a.obs = aobs; a.K = 1;
    a.P = aP; a.n = n_i; a.var_img = sigma_img * sigma_img; a.chi95 = h->d_chi95;
    a.A = nullptr; a.DB = 0; a.C1P = 0; a.na = n_i - XK_CORE;
    a.tile_rows = dint + 2; a.inlier = dint + 1; a.gamma = dscal + 2; a.gpf = dgpf + 4; a.gn_iters = dint + 3;
    a.gpf_in = dgpf; a.up_out = up + i * upsz; a.batch = nullptr; a.dbg = nullptr; a.inlier_h = nullptr; a.gamma_h = nullptr;
    a.gate_form = h->opt_gate_form;
    hipLaunchKernelGGL(xk_msckf_feature, dim3(1), dim3(XK_FEAT_THREADS), xk_feature_lds_bytes(np_i), h->stream, a);
    if (self) {
      int inl = 0;
      double g = 0;
      HIPCHK(h, hipMemcpyAsync(&inl, dint + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(&g, dscal + 2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      *self_inlier = inl;
      *self_gamma = g;
      if (!inl || k == 0) return XK_OK;  // proceed_with_multi_ false (:180)
    }
  }
  // null-space projection of the landmark and split into per-agent Jacobians (:207-223)
  XkCiProjArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.k1 = k1;
  pa.res = dres;
  for (int i = 0; i < k1; ++i) {
    pa.up[i] = up + i * upsz;
    pa.n[i] = (i == 0) ? n : m_n[i - 1];
    pa.H[i] = Hs + (size_t)m * nmax * i;
  }
  hipLaunchKernelGGL(xk_ci_project, dim3(k1), dim3(256), 0, h->stream, pa);
  // S_gate = sum H_i P_i H_i^T + sigma^2 I (:217-237) and the CI-weighted S (ci.cpp:78-85 + :255)
  const double w0 = 1.0 - (double)k * ci_msckf_w, var_img = sigma_img * sigma_img;
  for (int i = 0; i < k1; ++i) {
    const double *hP = (i == 0) ? P : m_P[i - 1];
    const int n_i = (i == 0) ? n : m_n[i - 1], ld_i = (i == 0) ? ldp : n_i;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, copy_matrix(h, aP, n_i, hP, ld_i, n_i, n_i, hipMemcpyHostToDevice));
    hp_product(h, pa.H[i], aP, m, n_i);  // W = H_i P_i, once for both outputs
    for (int pass = 0; pass < 2; ++pass) {  // 0: the gate's sum (weights play no part in it); 1: H_i P_i H_i^T on its own, weighted below
      XkGemmArgs g = wht_args(h, pa.H[i], m, n_i, pass ? ciw_T(h, i) : S1);
      g.beta = (i == 0 || pass) ? 0.0 : 1.0;
      g.mode = (i == k && !pass) ? 1 : 0;   // noise once, on the last term
      g.diag_scalar = var_img;
      gemm(h, g);
    }
    // searched weights: M_i = H_i P_i^-1 H_i^T while P_i is on the device -- one factorisation per agent
    if (srch)
      if (int rc = ci_info(h, pa.H[i], aP, m, n_i, ciw_M(h, i))) return rc;
  }
  hipLaunchKernelGGL(xk_small_gamma, dim3(1), dim3(1), 0, h->stream, S1, dres, m, dscal);
  double g_ci = 0;
  HIPCHK(h, hipMemcpyAsync(&g_ci, dscal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (srch)
    if (int rc = ciw_chol_status(h)) return rc;
  *ci_gamma = g_ci;
  if (!(g_ci < ci_gate_threshold(2 * Ltot - 3))) return XK_OK;   // :243-250
  // the CI-weighted S (ci.cpp:78-85 + :255): the weights sit in the entry's device slots, the host's constants or the searched ones
  if (!srch) {
    double v[XK_CIW_MAXK1] = {w0};
    for (int i = 1; i <= k; ++i) v[i] = ci_msckf_w;
    ciw_set(h, h->d_ciw, v, k1);
  } else {
    double st[XK_CIW_MAXK1];
    ciw_solve(h, m, k1, 576, ciw_start_multi(ci_msckf_w, k, st));
    if (int rc = ciw_fetch(h, k1, nullptr)) return rc;
  }
  for (int i = 0; i < k1; ++i) ciw_sum(h, ciw_T(h, i), S2, m, i, false, i == 0, i == k, var_img, i == 0 ? dscal + 1 : nullptr);
  // P_j: diagonal 3x3 blocks of the L observed poses scaled by w_result = 1/w0 (:256-267)
  std::vector<int> cols(2 * L);
  for (int i = 0; i < L; ++i) {
    const int pos = n_poses - L + i;
    cols[2 * i] = XK_CORE + 3 * pos;
    cols[2 * i + 1] = XK_CORE + 3 * pos + 3 * n_poses_max;
  }
  int *dcols = dint + 16;   // (dscal[1] = w_result = 1 / w_0 was left there by xk_ciw_sum)
  HIPCHK(h, hipMemcpyAsync(dcols, cols.data(), sizeof(int) * 2 * L, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, copy_matrix(h, h->d_tmpP, n, P, ldp, n, n, hipMemcpyHostToDevice));
  XkScaleArgs sc{h->d_tmpP, h->d_Pout, n, 2 * L, dcols, dscal + 1};
  hipLaunchKernelGGL(xk_scale_blocks, dim3(((size_t)n * n + 255) / 256), dim3(256), 0, h->stream, sc);
  HIPCHK(h, copy_matrix(h, H, ldh, pa.H[0], m, m, n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpyAsync(res, dres, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, copy_matrix(h, S, lds, S2, m, m, m, hipMemcpyDeviceToHost));
  HIPCHK(h, copy_matrix(h, P_j, ldpj, h->d_Pout, n, n, n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *has_ci = 1;
  return XK_OK;
}

// The search alone, on matrices the caller supplies (include/xk.h).
extern "C" int xk_ci_solve_weights(xk_handle *h, const double *M, int m, int k1, const double *w_start, double *w, int *iters) {
  if (!h || !M || !w) return XK_EINVAL;
  if (m < 1 || m > XK_CIW_MAXM || k1 < 2 || k1 > XK_CIW_MAXK1) return fail(h, XK_EINVAL, "xk_ci_solve_weights: 1 <= m <= 21, 2 <= k1 <= 8");
  if (w_start) {
    double sum = 0.0;
    for (int i = 0; i < k1; ++i) {
      if (!(w_start[i] >= XK_CIW_LB)) return fail(h, XK_EINVAL, "xk_ci_solve_weights: every start weight must be at least 1e-4");
      sum += w_start[i];
    }
    if (!(fabs(sum - 1.0) <= 1e-12)) return fail(h, XK_EINVAL, "xk_ci_solve_weights: the start weights must sum to one");
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(ciw_M(h, 0), M, sizeof(double) * (size_t)k1 * m * m, hipMemcpyHostToDevice, h->stream));
  ciw_solve(h, m, k1, m * m, w_start);
  if (int rc = ciw_fetch(h, k1, w)) return rc;
  if (iters) *iters = h->ci_last_iters;
  return XK_OK;
}

extern "C" int xk_ci_round_weights(const xk_handle *h, int track, double *w, int *k1, int *iters) {
  if (!h || !w || track < 0 || track >= h->ci_round_tracks) return XK_EINVAL;
  for (int i = 0; i < 8; ++i) w[i] = h->ci_round_w[track][i];
  if (k1) *k1 = h->ci_round_k1[track];
  if (iters) *iters = h->ci_round_iters[track];
  return XK_OK;
}

extern "C" int xk_ci_last_weights(const xk_handle *h, double *w, int *k1, int *iters) {
  if (!h || !w) return XK_EINVAL;
  for (int i = 0; i < 8; ++i) w[i] = h->ci_last_w[i];
  if (k1) *k1 = h->ci_last_k1;
  if (iters) *iters = h->ci_last_iters;
  return XK_OK;
}

// ---------------------------------------------------------------------------
// applyCI (updater.cpp:144-161) with a dense H and the CI-weighted S
// ---------------------------------------------------------------------------
// applyCI's UpdateSpec: T (m x n column-major, ld m), z (m) and the CI-weighted S (m x m, ld m) on the device, P <- Pout from Pin
static UpdateSpec ci_update_spec(const double *T, int m, int n, const double *z, const double *S, const double *Pin, double *Pout) {
  UpdateSpec u;
  memset(&u, 0, sizeof(u));
  u.T = T; u.str = 1; u.stc = m;
  u.c = m; u.kdim = n; u.col0 = 0;
  u.z = z; u.sz = 1;
  u.S = S; u.ssr = 1; u.ssc = m;
  u.Pin = Pin; u.Pout = Pout; u.ct = nullptr; u.cov_update = 1;
  return u;
}

// The two host entries: the operands into d_tmpP / d_tmpH / d_tmpS / d_tmpz, the update, the correction's copy queued behind it.
static int apply_ci_host(xk_handle *h, const double *ci_P, int ldc, int n, const double *H, int ldh, int m, const double *res,
                         const double *S, int lds, double *correction) {
  HIPCHK(h, copy_matrix(h, h->d_tmpP, n, ci_P, ldc, n, n, hipMemcpyHostToDevice));
  HIPCHK(h, copy_matrix(h, h->d_tmpH, m, H, ldh, m, n, hipMemcpyHostToDevice));
  HIPCHK(h, copy_matrix(h, h->d_tmpS, m, S, lds, m, m, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpyAsync(h->d_tmpz, res, sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
  const int rc = launch_update(h, ci_update_spec(h->d_tmpH, m, n, h->d_tmpz, h->d_tmpS, h->d_tmpP, h->d_Pout));
  if (rc != XK_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(correction, h->d_corr, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  return XK_OK;
}

extern "C" int xk_apply_ci(xk_handle *h, double *P_out, int ldp, const double *ci_P, int ldc, int n,
                           const double *H, int ldh, int m, const double *res, const double *S, int lds,
                           double *correction) {
  if (!h || !P_out || !ci_P || !H || !res || !S || !correction || n != h->n || ldp < n || ldc < n || ldh < m ||
      lds < m || m <= 0)
    return XK_EINVAL;
  if (m > h->CM) return fail(h, XK_ECAPACITY, "m exceeds the dense workspace");
  HIPCHK(h, hipSetDevice(h->device));
  const int rc = apply_ci_host(h, ci_P, ldc, n, H, ldh, m, res, S, lds, correction);
  if (rc != XK_OK) return rc;
  HIPCHK(h, copy_matrix(h, P_out, ldp, h->d_Pout, n, n, n, hipMemcpyDeviceToHost));
  return read_status(h);
}

// applyCI on the RESIDENT covariance: P <- sym((I - K H) ci_P) replaces the handle's covariance and stays on the
// device (the host mirror's resident mode; the compressed [T_H | z] of a pending xk_apply_update is not touched).
extern "C" int xk_apply_ci_resident(xk_handle *h, const double *ci_P, int ldc, int n, const double *H, int ldh, int m,
                                    const double *res, const double *S, int lds, double *correction) {
  if (!h || !ci_P || !H || !res || !S || !correction || n != h->n || ldc < n || ldh < m || lds < m || m <= 0) return XK_EINVAL;
  if (m > h->CM) return fail(h, XK_ECAPACITY, "m exceeds the dense workspace");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = settle_async(h);
  if (rc == XK_OK) rc = apply_ci_host(h, ci_P, ldc, n, H, ldh, m, res, S, lds, correction);
  if (rc == XK_OK) rc = read_status(h);
  if (rc != XK_OK) return rc;
  std::swap(h->d_P, h->d_Pout);
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Device-resident CI round: the gathered SimpleState payloads (and the observations of the shared
// tracks) stay where RCCL put them.  Same arithmetic as xk_msckf_ci_track + xk_apply_ci per shared
// track, with every per-agent stage batched over the agents and no host staging of the n x n
// covariances.  One host wait for the gate decisions of all tracks, one for the end of the round.
// ---------------------------------------------------------------------------
// A shared track's workspace, as offsets in doubles from the start of its region of d_ciws.  The stages before the gate of every
// shared track are queued back to back, so each track has a region of its own, sized for eight agents: ci_track_ws(n, 8).doubles.
//   dq, dp, dobs   the concatenated lists of the joint triangulation
//   up             per agent the column-space rows, upsz doubles each
//   Hs, Si, S1, S2 per-agent Jacobians; chunk partials of H_i P_i H_i^T; the gate's S; the CI-weighted S
//   dres, dgpf     residual; the landmark of the joint triangulation
//   dscal          [0] ci gamma, [1] w_result, [2..] per-agent gamma
//   dint           ints: [0..7] inlier per agent, [8..15] tile rows, [16..31] gn iters, [32..159] block columns, [192..] landmarks
//   doubles        the whole region
struct CiTrackWs { size_t dq, dp, dobs, up, upsz, Hs, Si, S1, S2, dres, dgpf, dscal, dint, doubles; };
static CiTrackWs ci_track_ws(int n, int k1) {
  const size_t Lcap = (size_t)k1 * 64, m = 3 * (size_t)(k1 - 1);
  CiTrackWs w;
  w.upsz = 3 * (size_t)n + 16;
  w.dq = 0; w.dp = w.dq + 4 * Lcap; w.dobs = w.dp + 3 * Lcap; w.up = w.dobs + 2 * Lcap;
  w.Hs = w.up + k1 * w.upsz; w.Si = w.Hs + std::max(m, (size_t)1) * k1 * n; w.S1 = w.Si + (size_t)k1 * XK_CI_MAXCHUNK * 576; w.S2 = w.S1 + 576;
  w.dres = w.S2 + 576; w.dgpf = w.dres + 24; w.dscal = w.dgpf + 8; w.dint = w.dscal + 16;
  w.doubles = w.dres + 512;   // (the words from dres on: 48 doubles and 256 ints)
  return w;
}

// The searched round's block d_ciwr, in doubles: per agent [Maug | X] (n x ld row-major each), then the solver's operands and results.
//   ld = n + 168 right-hand sides, agent = doubles per agent; then M [8 tracks][8 agents][576], start points [8][8], weights [8][8],
//   1 / w_0 [8], and as ints the solver's info words [8][2] and the pivot status per agent [8]
struct CiwrLayout { int ld; size_t agent, M, start, w, winv, info, status, doubles; };
static CiwrLayout ciwr_layout(int n) {
  CiwrLayout L;
  L.ld = n + XK_CIWR_MAXRHS;
  L.agent = 2 * (size_t)n * L.ld;
  L.M = XK_CIW_MAXK1 * L.agent; L.start = L.M + 64 * 576; L.w = L.start + 64; L.winv = L.w + 64;
  L.info = L.winv + 8; L.status = L.info + 8; L.doubles = L.status + 4;
  return L;
}

// What the stages of one round share.
//   srch: the weights are searched (ci_msckf_w < 0), else fixed: w0 own, w_oth every other agent (searched: xk_ci_combine runs with
//   unit weights); ci_seq: what the gate markers of this round hold; side: track j >= 1 runs its chain on ci_stream[j]; per track
//   its stream, the length of the own track and the threshold of the joint gate; ws: a track's region laid out for this
//   round's k1, region: the regions' spacing in d_ciws; as / fin: searched, filled track by track while the chains are prepared
struct CiRound {
  int world, self_rank, n_tracks, k, k1, m, n, N, srch;
  const double *d_payloads, *d_tracks;
  long payload_stride;
  const int *track_len, *n_poses_valid, *self_track;
  double ci_msckf_w, w0, w_oth, var_img;
  unsigned long long ci_seq;
  bool side;
  hipStream_t stream[8];
  int L0[8];
  double chi[8];
  CiTrackWs ws;
  size_t region;
  CiwrLayout wr;
  XkCiwrAssembleArgs as;
  XkCiwrFinishArgs fin;
};
static double *ci_round_ws(const xk_handle *h, const CiRound &r, int j) { return h->d_ciws + (size_t)j * r.region; }

// this track passed both gates: the own chi-square test (:180) and the joint one (:243-250)
static bool ci_round_passed(const xk_handle *h, const CiRound &r, int j) {
  const double *g = xk_cip_gate(h->h_ci_w, j);
  return g[0] != 0.0 && g[1] < r.chi[j];
}

// The agents of shared track j where their data lie on the device: index 0 = self (the staged problem), 1.. = the others by rank
// (their payloads and track observations).
struct CiTrackAgents { const double *q[XK_CI_MAXK + 1], *p[XK_CI_MAXK + 1], *obs[XK_CI_MAXK + 1], *P[XK_CI_MAXK + 1]; int np[XK_CI_MAXK + 1], L[XK_CI_MAXK + 1], Ltot; };
static void ci_round_agents(const xk_handle *h, const CiRound &r, int j, CiTrackAgents &ag) {
  // payload layout (fleet.py / xk_pack_payload): hdr[8] dyn[16] pos[3N] att[4N] feat[3M] anchors[M] cov[n*n]
  const size_t o_pos = 24, o_att = o_pos + 3 * (size_t)r.N, o_cov = o_att + 4 * (size_t)r.N + 4 * (size_t)h->Mmax;
  const size_t trk_stride = 1 + 2 * (size_t)r.N;
  const int st = r.self_track[j];
  ag.q[0] = h->d_q; ag.p[0] = h->d_p; ag.obs[0] = h->d_obs + 2 * (size_t)h->h_trk_off[st]; ag.P[0] = h->d_P;
  ag.np[0] = h->n_poses; ag.L[0] = h->h_trk_off[st + 1] - h->h_trk_off[st];
  for (int a = 0, i = 1; a < r.world; ++a) {
    if (a == r.self_rank) continue;
    const double *base = r.d_payloads + (size_t)a * r.payload_stride;
    ag.q[i] = base + o_att; ag.p[i] = base + o_pos; ag.P[i] = base + o_cov;
    ag.obs[i] = r.d_tracks + ((size_t)a * r.n_tracks + j) * trk_stride + 1;
    ag.np[i] = r.n_poses_valid[a]; ag.L[i] = r.track_len[a * r.n_tracks + j];
    ++i;
  }
  ag.Ltot = 0;
  for (int i = 0; i < r.k1; ++i) ag.Ltot += ag.L[i];
}

// Everything is validated BEFORE anything is queued or forked: an early return later would leave side streams running into
// workspace and pinned words the next call reuses.  Leaves every track's own length and joint-gate threshold in the record.
static int ci_round_validate(xk_handle *h, CiRound &r) {
  if (r.k > XK_CI_MAXK) return fail(h, XK_ECAPACITY, "more than 7 matched agents");
  if (r.self_rank < 0 || r.self_rank >= r.world || r.n_tracks < 0 || r.n_tracks > 8) return XK_EINVAL;
  if (r.payload_stride != xk_payload_doubles(r.N, h->Mmax)) return fail(h, XK_EINVAL, "payload layout differs from this handle's (N, M)");
  if (h->n_poses < 2) return fail(h, XK_EINVAL, "window not staged");
  if (check_w(h, r.ci_msckf_w) < 0)
    return fail(h, XK_EINVAL, (r.ci_msckf_w < 0 && r.ci_msckf_w >= -1 && !h->opt_ci_search)
                                  ? "xk_ci_round_device: a negative CI weight asks for the weight search, which is switched off (xk_set_option \"ci_weight_search\", 1)"
                                  : "The CI weights must be lower than 1.0 and larger 0.0");
  if (r.m > h->CM) return fail(h, XK_ECAPACITY, "m exceeds the dense workspace");
  for (int j = 0; j < r.n_tracks; ++j) {
    const int st = r.self_track[j];
    if (st < 0 || st >= h->K) return fail(h, XK_EINVAL, "shared track index outside the staged tracks");
    CiTrackAgents ag;
    ci_round_agents(h, r, j, ag);
    for (int i = 1; i < r.k1; ++i)
      if (ag.L[i] < 2 || ag.L[i] > ag.np[i] || ag.np[i] > r.N) return fail(h, XK_EINVAL, "received track / window lengths inconsistent");
    r.L0[j] = ag.L[0];
    r.chi[j] = ci_gate_threshold(2 * ag.Ltot - 3);
  }
  return XK_OK;
}

// The round's resources, each created if it is not there yet: a call after one that failed half way completes the set.
static int ci_round_resources(xk_handle *h, const CiRound &r) {
  if (!h->d_ciws) {
    hipFuncSetAttribute((const void *)xk_ci_hph, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    HIPCHK(h, hipMalloc((void **)&h->d_ciws, sizeof(double) * 8 * r.region));   // one region per shared track
  }
  if (!h->d_batch) HIPCHK(h, hipMalloc((void **)&h->d_batch, sizeof(XkFeatBatch) * 64));
  if (!h->h_batch) HIPCHK(h, hipHostMalloc((void **)&h->h_batch, sizeof(XkFeatBatch) * 64));
  if (!h->h_ci_w) {
    HIPCHK(h, hipHostMalloc((void **)&h->h_ci_w, sizeof(double) * XK_CIP_DOUBLES));
    memset(h->h_ci_w, 0, sizeof(double) * XK_CIP_DOUBLES);
  }
  if (!h->ci_fork) HIPCHK(h, hipEventCreateWithFlags(&h->ci_fork, hipEventDisableTiming));
  for (int j = 1; j < 8; ++j) {
    if (!h->ci_stream[j]) HIPCHK(h, hipStreamCreateWithFlags(&h->ci_stream[j], hipStreamNonBlocking));
    if (!h->ci_join[j]) HIPCHK(h, hipEventCreateWithFlags(&h->ci_join[j], hipEventDisableTiming));
  }
  if (r.srch && !h->d_ciwr) HIPCHK(h, hipMalloc((void **)&h->d_ciwr, sizeof(double) * r.wr.doubles));
  return XK_OK;
}

// A HIP error after the fork: the side streams are joined before the error is returned.
static int ci_round_bail(xk_handle *h, int rc) {
  for (int j = 1; j < 8; ++j)
    if (h->ci_stream[j]) hipStreamSynchronize(h->ci_stream[j]);
  hipStreamSynchronize(h->stream);
  return rc;
}
#define CI_ROUND_CHK(h, call)                                                                   \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return ci_round_bail((h), fail((h), XK_EDEVICE, #call, e_));          \
  } while (0)

typedef std::vector<std::function<hipError_t()>> CiStage;   // one stage of the chain: a prepared call per track

// One track's chain, PREPARED: stage s of it goes to the back of stage[s].  Round 6: the launches are issued stage by stage over all
// tracks afterwards.  The round was bound by the host issuing 2 x 8 launches one track after the other (~7 us each: the second
// track's chain started 60 us after the first one's, tools/exp/ci_round_kernels.sh); stage-major, both chains are in flight from
// the first launch on.
static void ci_round_prepare(xk_handle *h, CiRound &r, int j, CiStage (&stage)[8]) {
  const int k = r.k, k1 = r.k1, m = r.m, n = r.n, N = r.N;
  const hipStream_t sj = r.stream[j];
  const CiTrackWs &w = r.ws;
  double *ws = ci_round_ws(h, r, j);
  double *dq = ws + w.dq, *dp = ws + w.dp, *dobs = ws + w.dobs, *up = ws + w.up, *Hs = ws + w.Hs, *Si = ws + w.Si, *S1 = ws + w.S1;
  double *S2 = ws + w.S2, *dres = ws + w.dres, *dgpf = ws + w.dgpf, *dscal = ws + w.dscal;
  int *dint = (int *)(ws + w.dint);
  CiTrackAgents ag;
  ci_round_agents(h, r, j, ag);
  // joint triangulation over the concatenated lists: matched agents first, self last (:113-149)
  XkCiGatherArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.k1 = k1; ga.dq = dq; ga.dp = dp; ga.dobs = dobs;
  for (int i = 0; i < k1; ++i) {
    const int src = (i < k) ? i + 1 : 0;
    ga.q[i] = ag.q[src]; ga.p[i] = ag.p[src]; ga.obs[i] = ag.obs[src]; ga.np[i] = ag.np[src]; ga.L[i] = ag.L[src];
  }
  stage[0].push_back([=]() { hipLaunchKernelGGL(xk_ci_gather, dim3(k1), dim3(64), 0, sj, ga); return hipSuccess; });
  XkTriMultiArgs ta{dq, dp, dobs, ag.Ltot, dgpf, dint + 16, nullptr, 0};
  stage[1].push_back([=]() { hipLaunchKernelGGL(xk_triangulate_multi, dim3(1), dim3(64), 0, sj, ta); return hipSuccess; });
  // per-agent column-space rows, one workgroup per agent (:168-204)
  XkFeatBatch *hb = h->h_batch + 8 * j, *db = h->d_batch + 8 * j;
  int npmax = 0;
  for (int i = 0; i < k1; ++i) {
    hb[i].q = ag.q[i]; hb[i].p = ag.p[i]; hb[i].obs = ag.obs[i]; hb[i].P = ag.P[i];
    hb[i].n_poses = ag.np[i]; hb[i].n_poses_max = N; hb[i].n = n; hb[i].L = ag.L[i]; hb[i].up_out = up + i * w.upsz;
    npmax = std::max(npmax, ag.np[i]);
  }
  stage[2].push_back([=]() { return hipMemcpyAsync(db, hb, sizeof(XkFeatBatch) * k1, hipMemcpyHostToDevice, sj); });
  XkFeatArgs a;
  memset(&a, 0, sizeof(a));
  a.K = k1; a.var_img = r.var_img; a.chi95 = h->d_chi95; a.n = n; a.na = n - XK_CORE; a.n_poses = npmax; a.n_poses_max = N;
  a.tile_rows = dint + 8; a.inlier = dint; a.gamma = dscal + 2; a.gpf = (double *)(dint + 192); a.gn_iters = dint + 24;
  a.gpf_in = dgpf; a.batch = db; a.gate_form = h->opt_gate_form;
  stage[3].push_back([=]() { hipLaunchKernelGGL(xk_msckf_feature, dim3(k1), dim3(XK_FEAT_THREADS), xk_feature_lds_bytes(npmax), sj, a); return hipSuccess; });
  // null-space projection of the landmark and split into per-agent Jacobians (:207-223)
  XkCiProjArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.k1 = k1; pa.res = dres;
  for (int i = 0; i < k1; ++i) { pa.up[i] = up + i * w.upsz; pa.n[i] = n; pa.H[i] = Hs + (size_t)m * n * i; }
  stage[4].push_back([=]() { hipLaunchKernelGGL(xk_ci_project, dim3(k1), dim3(256), 0, sj, pa); return hipSuccess; });
  // S_i = H_i P_i H_i^T for all agents, then the gate / CI combinations and gamma
  XkCiHphArgs ha;
  memset(&ha, 0, sizeof(ha));
  ha.m = m; ha.S = Si;
  for (int i = 0; i < k1; ++i) { ha.H[i] = pa.H[i]; ha.P[i] = ag.P[i]; ha.n[i] = n; }
  const int nchunk = (n + XK_CI_CHUNK - 1) / XK_CI_CHUNK;
  stage[5].push_back([=]() { hipLaunchKernelGGL(xk_ci_hph, dim3(k1, nchunk), dim3(256), sizeof(double) * ((size_t)m * n + 24 * 33), sj, ha); return hipSuccess; });
  // the two gate decisions (own chi-square test :180, joint test :243-250) come back per track: written by the kernel into
  // pinned host memory, a marker behind them
  // (searched: the gate words and the marker come from the last kernel of the searched chain instead)
  XkCiCombineArgs ca{k1, m, Si, nchunk, r.w0, r.w_oth, r.var_img, dres, S1, S2, dscal,
                     dint, xk_cip_gate(h->h_ci_w, j), r.srch ? nullptr : xk_cip_marker(h->h_ci_w, j), r.ci_seq};
  if (r.srch) {
    r.as.H[j] = Hs;
    if (j == 0)
      for (int i = 0; i < k1; ++i) r.as.P[i] = ag.P[i];
    r.fin.Si[j] = Si; r.fin.S_ci[j] = S2; r.fin.own_inlier[j] = dint; r.fin.gamma[j] = dscal;
  }
  stage[6].push_back([=]() { hipLaunchKernelGGL(xk_ci_combine, dim3(1), dim3(512), 0, sj, ca); return hipSuccess; });
  if (r.side && j > 0) {
    hipEvent_t ej = h->ci_join[j];
    hipStream_t s0 = h->stream;
    stage[7].push_back([=]() { hipError_t e = hipEventRecord(ej, sj); return e != hipSuccess ? e : hipStreamWaitEvent(s0, ej, 0); });
  }
}

// Fork, prepare every track's chain, issue stage-major.  The shared tracks are independent until applyCI (every P_j is built from
// the same prior), and a track's stages are a chain of seven small launches (~160 us at 8 agents): track j >= 1 runs its chain on a
// side stream next to track 0's.
static int ci_round_issue(xk_handle *h, CiRound &r) {
  if (r.side) CI_ROUND_CHK(h, hipEventRecord(h->ci_fork, h->stream));
  CiStage stage[8];
  for (int j = 0; j < r.n_tracks; ++j) {
    if (r.side && j > 0) CI_ROUND_CHK(h, hipStreamWaitEvent(r.stream[j], h->ci_fork, 0));
    ci_round_prepare(h, r, j, stage);
  }
  for (auto &s : stage)
    for (auto &issue : s) CI_ROUND_CHK(h, issue());
  return XK_OK;
}

// The searched chain, on the engine's stream behind the join of the side streams (it needs every track's Jacobians): the
// information projections of all agents and tracks with ONE factorisation per agent, the search per track, the weighted S_ci.
static int ci_round_search(xk_handle *h, CiRound &r) {
  const int n = r.n, m = r.m, k1 = r.k1, n_tracks = r.n_tracks;
  const CiwrLayout &L = r.wr;
  double *ciwr_M = h->d_ciwr + L.M, *ciwr_start = h->d_ciwr + L.start, *ciwr_w = h->d_ciwr + L.w, *ciwr_winv = h->d_ciwr + L.winv;
  int *ciwr_info = (int *)(h->d_ciwr + L.info), *ciwr_status = (int *)(h->d_ciwr + L.status);
  XkCiwrAgents ag;
  memset(&ag, 0, sizeof(ag));
  ag.ld = L.ld;
  for (int i = 0; i < k1; ++i) { ag.Maug[i] = h->d_ciwr + (size_t)i * L.agent; ag.X[i] = ag.Maug[i] + (size_t)n * L.ld; }
  const int ncols = n + n_tracks * m;
  double st[XK_CIW_MAXK1];
  const double *start = ciw_start_multi(r.ci_msckf_w, r.k, st);
  r.as.ag = ag; r.as.n = n; r.as.m = m; r.as.k1 = k1; r.as.nt = n_tracks;
  r.as.start = start ? ciwr_start : nullptr; r.as.status = ciwr_status;
  for (int i = 0; i < XK_CIW_MAXK1; ++i) r.as.st[i] = (start && i < k1) ? st[i] : 0.0;
  hipLaunchKernelGGL(xk_ciwr_assemble, dim3((unsigned)(((size_t)n * ncols + 255) / 256), k1), dim3(256), 0, h->stream, r.as);
  const int B = 16 * XK_CHOLW_MAXB;
  for (int off = 0; off < n;) {
    const int cb = std::min(B, n - off);
    XkCiwrCholArgs d;
    d.ag = ag; d.off = off; d.c = cb; d.ncols = ncols - off; d.status = ciwr_status;
    xk_cholw_table((cb + 15) / 16, d.tab);
    hipLaunchKernelGGL(xk_ciwr_chol, dim3((ncols - off - cb + 15) / 16, k1), dim3(64 * XK_CHOLW_WAVES), 0, h->stream, d);
    off += cb;
    if (off < n) {
      XkCiwrSchurArgs sa{ag, off, cb, n - off, ncols - off};
      hipLaunchKernelGGL(xk_ciwr_schur, dim3((ncols - off + 15) / 16, (n - off + 15) / 16, k1), dim3(64), 0, h->stream, sa);
    }
  }
  XkCiwrXtxArgs xa{ag, n, m, ciwr_M};
  hipLaunchKernelGGL(xk_ciwr_xtx, dim3(n_tracks, k1), dim3(256), 0, h->stream, xa);
  // (no handle status word: a failing problem on a track the gates reject must not poison the handle)
  XkCiwArgs wa{ciwr_M, (long)XK_CIW_MAXK1 * 576, 576, m, k1, start ? ciwr_start : nullptr, ciwr_w, ciwr_info, nullptr, 1};
  hipLaunchKernelGGL(xk_ci_weights, dim3(n_tracks), dim3(XK_CIW_THREADS), 0, h->stream, wa);
  r.fin.nt = n_tracks; r.fin.k1 = k1; r.fin.m = m; r.fin.nchunk = (n + XK_CI_CHUNK - 1) / XK_CI_CHUNK;
  r.fin.var_img = r.var_img; r.fin.w = ciwr_w; r.fin.info = ciwr_info; r.fin.status = ciwr_status;
  r.fin.winv = ciwr_winv; r.fin.host = h->h_ci_w; r.fin.seq = r.ci_seq;
  hipLaunchKernelGGL(xk_ciwr_finish, dim3(1), dim3(512), 0, h->stream, r.fin);
  CI_ROUND_CHK(h, hipGetLastError());
  return XK_OK;
}

// wait for the markers of all tracks (XK_SPIN_DONE=0, or a marker that does not come within ~1 s: the runtime's signal)
static int ci_round_wait_gates(xk_handle *h, const CiRound &r) {
  bool seen = spin_done() != 0;
  for (int j = 0; j < r.n_tracks && seen; ++j) seen = wait_marker(h, xk_cip_marker(h->h_ci_w, j), r.ci_seq);
  if (!seen) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int j = 1; j < r.n_tracks && r.side; ++j) HIPCHK(h, hipStreamSynchronize(h->ci_stream[j]));
  }
  return XK_OK;
}

// What the searched chain left in pinned memory with the gate words.  No silent fallback: a covariance that is not positive
// definite fails the round whatever the gates say (as the host route, which checks before the gate decision), and so does a
// failed search on a track that passes both gates.  Nothing has been applied at this point.  Then the weights of the fused
// tracks are kept for xk_ci_round_weights / xk_ci_last_weights.
static int ci_round_search_results(xk_handle *h, const CiRound &r) {
  const int *pst = xk_cip_status(h->h_ci_w), *pinfo = xk_cip_info(h->h_ci_w);
  for (int i = 0; i < r.k1; ++i)
    if (pst[i] != 0) {
      const int rank = i == 0 ? r.self_rank : (i - 1 < r.self_rank ? i - 1 : i);
      char msg[128];
      snprintf(msg, sizeof(msg), "CI weight search: the covariance of the agent of rank %d is not positive definite", rank);
      return fail(h, XK_ESINGULAR, msg);
    }
  for (int j = 0; j < r.n_tracks; ++j)
    if (ci_round_passed(h, r, j) && pinfo[2 * j + 1] != 0) return ciw_search_failed(h, pinfo[2 * j]);
  h->ci_round_tracks = r.n_tracks;
  int last_fused = -1;
  for (int j = 0; j < r.n_tracks; ++j) {
    const bool pass = ci_round_passed(h, r, j);
    for (int i = 0; i < 8; ++i) h->ci_round_w[j][i] = (pass && i < r.k1) ? xk_cip_weights(h->h_ci_w, j)[i] : 0.0;
    h->ci_round_k1[j] = pass ? r.k1 : 0;
    h->ci_round_iters[j] = pass ? pinfo[2 * j] : 0;
    if (pass) last_fused = j;
  }
  if (last_fused >= 0) {
    memcpy(h->ci_last_w, h->ci_round_w[last_fused], sizeof(h->ci_last_w));
    h->ci_last_k1 = r.k1;
    h->ci_last_iters = h->ci_round_iters[last_fused];
  }
  return XK_OK;
}

// applyCI (updater.cpp:144-161) for every track that passed, in track order: every entry starts from the same prior and
// overwrites the posterior, so the last fused entry is the resident covariance afterwards.
static int ci_round_apply(xk_handle *h, const CiRound &r, double *corrections, int *n_fused) {
  const int n = r.n, m = r.m;
  int fused = 0, last_fused = -1;
  for (int j = 0; j < r.n_tracks; ++j)
    if (ci_round_passed(h, r, j)) last_fused = j;
  unsigned long long *done = reinterpret_cast<unsigned long long *>(h->h_out + h->n + 2);
  unsigned long long wait_seq = 0;
  for (int j = 0; j < r.n_tracks; ++j) {
    if (!ci_round_passed(h, r, j)) continue;
    double *ws = ci_round_ws(h, r, j);
    // P_j: diagonal 3x3 blocks of the observed poses scaled by 1/w0 (:256-267)
    // (the blocks are those of the last L window poses: the kernel works their columns out itself -- no staging copies)
    // (searched: the factor is the device word 1 / w_0 the searched chain left for this track)
    const int L = r.L0[j];
    XkScaleArgs sc{h->d_P, h->d_tmpP, n, 2 * L, nullptr, nullptr, 1, h->n_poses - L, L, r.N, 1.0 / r.w0, r.srch ? h->d_ciwr + r.wr.winv + j : nullptr};
    hipLaunchKernelGGL(xk_scale_blocks, dim3(((size_t)n * n + 255) / 256), dim3(256), 0, h->stream, sc);
    UpdateSpec u = ci_update_spec(ws + r.ws.Hs, m, n, ws + r.ws.dres, ws + r.ws.S2, h->d_tmpP, h->d_Pout);   // H of agent 0 (self)
    if (j == last_fused && !corrections && spin_done()) { u.done_flag = done; u.done_seq = wait_seq = ++h->done_seq; }   // the round's last launch marks its end
    int rc = launch_update(h, u);
    if (rc != XK_OK) return rc;
    if (corrections) HIPCHK(h, hipMemcpyAsync(corrections + (size_t)fused * n, h->d_corr, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    ++fused;                                       // (read_status below waits)
  }
  if (fused) {
    // (as xk_apply_update: the marker is the last store of the last kernel; a status word ends the wait early)
    const bool seen = wait_seq && wait_marker(h, done, wait_seq);
    int rc;
    if (seen) { h->done_seen = wait_seq; stage_stream_idle(h); rc = eval_status(h, h->d_status[0], h->d_status[1], false); }
    else rc = read_status(h);
    if (rc != XK_OK) return rc;
    std::swap(h->d_P, h->d_Pout);
    pending_drop(h);
  }
  *n_fused = fused;
  return XK_OK;
}

extern "C" int xk_ci_round_device(xk_handle *h, const double *d_payloads, long payload_stride, int world, int self_rank,
                                  const double *d_tracks, int n_tracks, const int *track_len, const int *n_poses_valid,
                                  const int *self_track, double sigma_img, double ci_msckf_w, int *n_fused,
                                  double *corrections) {
  if (!h || !d_payloads || !d_tracks || !track_len || !n_poses_valid || !self_track || !n_fused) return XK_EINVAL;
  *n_fused = 0;
  if (world < 2) return XK_OK;
  CiRound r;
  memset(&r, 0, sizeof(r));
  r.world = world; r.self_rank = self_rank; r.n_tracks = n_tracks;
  r.k = world - 1; r.k1 = world; r.m = 3 * r.k; r.n = h->n; r.N = h->N;
  r.d_payloads = d_payloads; r.d_tracks = d_tracks; r.payload_stride = payload_stride;
  r.track_len = track_len; r.n_poses_valid = n_poses_valid; r.self_track = self_track;
  r.ci_msckf_w = ci_msckf_w;
  int rc = ci_round_validate(h, r);
  if (rc != XK_OK) return rc;
  r.srch = check_w(h, ci_msckf_w);
  // (searched: xk_ci_combine's own S_ci is formed with unit weights and replaced by xk_ciwr_finish)
  r.w0 = r.srch ? 1.0 : 1.0 - (double)r.k * ci_msckf_w; r.w_oth = r.srch ? 1.0 : ci_msckf_w; r.var_img = sigma_img * sigma_img;
  r.ws = ci_track_ws(r.n, r.k1);
  r.region = ci_track_ws(r.n, XK_CIW_MAXK1).doubles;
  r.wr = ciwr_layout(r.n);
  static const int side_env = env_int("XK_CI_SIDE_STREAMS", 1);
  r.side = side_env && n_tracks > 1;
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = ci_round_resources(h, r)) != XK_OK) return rc;
  if ((rc = flush_window(h)) != XK_OK) return rc;
  for (int j = 0; j < n_tracks; ++j) r.stream[j] = (r.side && j > 0) ? h->ci_stream[j] : h->stream;
  r.ci_seq = ++h->done_seq;
  if ((rc = ci_round_issue(h, r)) != XK_OK) return rc;
  if (n_tracks == 0) return XK_OK;
  if (r.srch && (rc = ci_round_search(h, r)) != XK_OK) return rc;
  if ((rc = ci_round_wait_gates(h, r)) != XK_OK) return rc;
  if (r.srch && (rc = ci_round_search_results(h, r)) != XK_OK) return rc;
  return ci_round_apply(h, r, corrections, n_fused);
}

// ---------------------------------------------------------------------------
// inter-agent payload
// ---------------------------------------------------------------------------
extern "C" long xk_payload_doubles(int N, int M) {
  const long n = XK_CORE + 6L * N + 3L * M;
  return 8 + 16 + 3L * N + 4L * N + 3L * M + M + n * n;
}

__global__ void xk_pack_small(const double *hdr_dyn /*24*/, const double *p, const double *q, int n_poses,
                              const double *feat, const int *anchors, int Mcur, int N, int M, double *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int o_pos = 24, o_att = o_pos + 3 * N, o_feat = o_att + 4 * N, o_anc = o_feat + 3 * M, o_cov = o_anc + M;
  if (i >= o_cov) return;
  double v = 0.0;
  if (i < 24) v = hdr_dyn[i];
  else if (i < o_att) { const int t = i - o_pos; v = (t < 3 * n_poses) ? p[t] : 0.0; }
  else if (i < o_feat) { const int t = i - o_att; v = (t < 4 * n_poses) ? q[t] : 0.0; }
  else if (i < o_anc) { const int t = i - o_feat; v = (t < 3 * Mcur) ? feat[t] : 0.0; }
  else { const int t = i - o_anc; v = (t < Mcur) ? (double)anchors[t] : -1.0; }
  out[i] = v;
}

extern "C" int xk_pack_payload(xk_handle *h, double agent_id, double timestamp, const double *dyn16,
                               double *d_dst, double **d_payload) {
  if (!h || !dyn16) return XK_EINVAL;
  double *dst = d_dst ? d_dst : h->d_payload;
  HIPCHK(h, hipSetDevice(h->device));
  { int rcw = flush_window(h); if (rcw != XK_OK) return rcw; }
  double *hd = h->h_pin;
  hd[0] = agent_id; hd[1] = timestamp; hd[2] = h->N; hd[3] = h->Mmax; hd[4] = h->n; hd[5] = h->n_poses;
  hd[6] = 0.0; hd[7] = 0.0;
  for (int i = 0; i < 16; ++i) hd[8 + i] = dyn16[i];
  HIPCHK(h, hipMemcpyAsync(h->d_ci, hd, sizeof(double) * 24, hipMemcpyHostToDevice, h->stream));
  const int small = 24 + 7 * h->N + 4 * h->Mmax;
  hipLaunchKernelGGL(xk_pack_small, dim3((small + 255) / 256), dim3(256), 0, h->stream, h->d_ci, h->d_p, h->d_q,
                     h->n_poses, h->d_feat, h->d_anchor, h->M, h->N, h->Mmax, dst);
  HIPCHK(h, hipMemcpyAsync(dst + small, h->d_P, sizeof(double) * (size_t)h->n * h->n,
                           hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (d_payload) *d_payload = dst;
  return XK_OK;
}
