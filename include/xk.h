/*
 * xk.h -- C ABI of the MI355X-native xVIO EKF-update engine.
 *
 * This is the drop-in boundary for ONE path of jpl-x/x_multi_agent: the
 * visual EKF update (MSCKF build -> QR compression -> Kalman update) and the
 * covariance-intersection fusion step.  Each entry point names the reference
 * interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - all matrices are column-major IEEE doubles with an explicit leading
 *     dimension (Eigen::MatrixXd::data() can be passed directly);
 *   - quaternions are (x,y,z,w) as stored in State::q_array_
 *     (src/x/ekf/state.cpp:235-240);
 *   - error-state column map (include/x/common/types.h:39-47,
 *     msckf_update.cpp:412-416): [0,15) core, 15+3i position of window pose
 *     i, 15+3N+3i attitude of pose i, 15+6N+3j SLAM feature j;
 *   - the caller owns every host buffer; the library never keeps a host
 *     pointer after a call returns; device memory belongs to the handle;
 *   - one handle per agent / x::Ekf; calls on one handle are serialised by
 *     the caller (as Updater::update is in the reference, ekf.cpp:186-205),
 *     distinct handles are independent;
 *   - every call is synchronous unless its name ends in _async;
 *   - return value is an xk_status; nothing aborts, nothing throws.
 */
#ifndef XK_H_
#define XK_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xk_handle xk_handle;

typedef enum {
  XK_OK = 0,
  XK_EINVAL = 1,    /* bad dims / CI weights (ci.cpp:59-62,98-101 throw) */
  XK_ESINGULAR = 2, /* innovation covariance not SPD */
  XK_ENAN = 3,
  XK_EDEVICE = 4,   /* HIP runtime error; see xk_last_error */
  XK_ENOMEM = 5,
  XK_ECAPACITY = 6  /* problem larger than the handle was created for */
} xk_status;

#define XK_CORE 15 /* kSizeCoreErr, include/x/common/types.h:45 */

/* ---- lifetime -------------------------------------------------------- */

/* Creates the per-agent engine on HIP device `device`.  Capacities:
 * n_poses_max = sliding-window length N (Params::n_poses_max,
 * include/x/vio/types.h), n_feat_max = SLAM feature slots M, k_max = MSCKF
 * tracks per update.  n = 15 + 6N + 3M. */
int xk_create(int device, int n_poses_max, int n_feat_max, int k_max, xk_handle **out);
int xk_destroy(xk_handle *h);
const char *xk_strerror(int status);
const char *xk_last_error(const xk_handle *h);
int xk_version(void);
/* HIP stream the handle launches on (void* = hipStream_t), for callers that
 * want to order their own device work or time with events. */
void *xk_stream(xk_handle *h);

/* ---- staged (device-resident) visual update -------------------------- */

/* Stage the inputs of one visual update in HBM.  Replaces the arguments of
 * the MsckfUpdate / SlamUpdate constructors as called from
 * VioUpdater::constructUpdate (src/x/vio/vio_updater.cpp:279-305,338-346):
 *   C_q_G [n_poses x 4] xyzw, G_p_C [n_poses x 3]   window lists
 *       (StateManager::convertCamera{Attitudes,Positions}ToList,
 *        src/x/vio/state_manager.cpp:539-584), row per pose;
 *   trk_off [K+1], obs_xy [trk_off[K] x 2]          MSCKF tracks, normalised
 *       image coordinates (Feature::getX/getY); a length-L track observes the
 *       LAST L window poses (msckf_update.cpp:329-331);
 *   P [n x n], ldp                                  prior covariance
 *       (Matrix P = state.getCovariance(), vio_updater.cpp:284);
 *   SLAM (M may be 0): feat [3M] inverse-depth states, anchor_idxs [M],
 *       track_sizes [M] >= 1 (only used for the chi-square dof 2 * size,
 *       slam_update.cpp:196; no upper limit -- a persistent feature's track
 *       grows every frame: the 0.9 quantile comes from a table below dof 513
 *       and is computed on the host past it), z_last [M x 2] newest
 *       observation. */
int xk_stage_window(xk_handle *h, const double *C_q_G, const double *G_p_C, int n_poses);
int xk_stage_tracks(xk_handle *h, const int *trk_off, const double *obs_xy, int K);
/* The same in two halves for a host that builds the CSR lists anyway: *trk_off (K+1 ints) and *obs_xy (2 n_obs doubles)
 * point INTO the handle's pinned staging memory; fill them, then call xk_stage_tracks_end (which validates like
 * xk_stage_tracks and queues the one copy).  Replaces the list -> vector -> staging double copy of a C++ host
 * (host/src/vio_updater.cpp, mirror of the list walk in vio_updater.cpp:267-300). */
int xk_stage_tracks_begin(xk_handle *h, int K, int n_obs, int **trk_off, double **obs_xy);
int xk_stage_tracks_end(xk_handle *h);
int xk_stage_slam(xk_handle *h, const double *feat, const int *anchor_idxs, const int *track_sizes,
                  const double *z_last, int M);
/* boost::math::quantile(chi_squared(dof), p) as xk_stage_slam computes it past its table (0 < p < 1, dof >= 1); no handle, no
 * device. */
int xk_chi2_quantile(double p, int dof, double *out);
int xk_upload_P(xk_handle *h, const double *P, int ldp, int n);
int xk_download_P(xk_handle *h, double *P, int ldp, int n);

/* Per-feature build on the staged inputs: triangulation (triangulation.cpp:
 * 48-206), Jacobians + observability constraint + left-nullspace projection +
 * chi-square gate (msckf_update.cpp:65-173,283-492), SLAM rows
 * (slam_update.cpp:49-214).  Leaves the projected rows [H0|res0]
 * device-resident.  Outputs (host, optional = NULL): inlier/gamma per track. */
int xk_msckf_build(xk_handle *h, double sigma_img, int *inlier_msckf, double *gamma_msckf,
                   int *inlier_slam, double *gamma_slam);

/* Householder QR (communication-avoiding, panel by panel) of the device-resident stacked [H|res]; replaces
 * VioUpdater::applyQRDecomposition (vio_updater.cpp:487-512).  Optional host
 * outputs: T_H (n x n, ldt; upper-trapezoidal, zero core columns) and z (n).
 * T_H^T T_H and T_H^T z equal the reference's up to rounding; the rows
 * themselves differ by an orthogonal factor. */
int xk_qr_compress(xk_handle *h, double *T_H, int ldt, double *z);

/* Kalman gain + covariance/state-correction on the compressed system with
 * R = sigma_img^2 I; replaces Updater::applyUpdate (src/x/ekf/updater.cpp:
 * 117-141): S = HPH^T+R, K = PH^T S^-1, corr = K(res + H corr_tot) - corr_tot,
 * P = (I-KH)P, P = (P+P^T)/2.  P stays on the device (xk_download_P);
 * correction (n) is returned to the host because State::correct
 * (state.cpp:197-249) runs there.  corr_total may be NULL (= 0). */
int xk_apply_update(xk_handle *h, const double *corr_total, int cov_update, double *correction);

/* xk_msckf_build + xk_qr_compress + xk_apply_update in one call on the staged
 * inputs, no host round trips in between (a5..a12 of SURVEY 8a). */
int xk_visual_update_staged(xk_handle *h, double sigma_img, double *correction, int *inlier_msckf,
                            double *gamma_msckf, int *inlier_slam, double *gamma_slam);

/* Convenience: stage + update + download in one call (host buffers in/out;
 * PCIe inclusive).  P is updated in place. */
int xk_visual_update(xk_handle *h, const double *C_q_G, const double *G_p_C, int n_poses,
                     const int *trk_off, const double *obs_xy, int K, const double *feat,
                     const int *anchor_idxs, const int *track_sizes, const double *z_last, int M,
                     double *P, int ldp, int n, double sigma_img, double *correction,
                     int *inlier_msckf, double *gamma_msckf, int *inlier_slam, double *gamma_slam);

/* ---- dense (unfused) Kalman algebra, reference signatures ------------ */

/* Updater::applyUpdate(state, H, res, R, correction_total, cov_update) with
 * arbitrary dense H (m x n) and diagonal R (updater.cpp:117-141).  P in/out
 * on the host; correction_total (n) in/out (updater.cpp:140). */
int xk_apply_update_dense(xk_handle *h, double *P, int ldp, int n, const double *H, int ldh, int m,
                          const double *res, const double *r_diag, double *correction_total,
                          int cov_update, double *correction);

/* Updater::applyCI(state, ci_P, H, res, S) (updater.cpp:144-161):
 * K = ci_P H^T S^-1, corr = K res, P_out = sym((I-KH) ci_P).
 * S and ci_P are taken as symmetric, S positive definite (what the CI entries produce from a
 * covariance): S is factored by Cholesky, ONE of its triangles is read, and an S that is not
 * positive definite is XK_ESINGULAR.  The reference inverts S as a general matrix; on an S whose
 * two triangles differ by 4e-8 (relative) the two disagree by 4e-7 on P_out
 * (tests/test_ci_entry_cases.py). */
int xk_apply_ci(xk_handle *h, double *P_out, int ldp, const double *ci_P, int ldc, int n,
                const double *H, int ldh, int m, const double *res, const double *S, int lds,
                double *correction);

/* ---- covariance intersection (fixed or searched weights) ------------- */

/* The weight argument of the five CI entries below (xk_fuse_ci_msckf, xk_fuse_ci_slam, xk_multi_slam_match,
 * xk_msckf_ci_track, xk_ci_round_device) follows CovarianceIntersection::fuseCI (src/x/ekf/ci.cpp):
 *   0 < w <= 1     fixed weights.
 *   w > 1, w == 0, w < -1   XK_EINVAL (the reference throws, ci.cpp:59-62,98-101).
 *   -1 <= w < 0    "search the weights" (ci.cpp:65-73,105-119 -> solveW, :143-190).  XK_EINVAL unless
 *                  xk_set_option(h, "ci_weight_search", 1) was called (default 0).
 * The search minimises the reference's objective under the reference's bounds,
 *   det((sum_i w_i M_i)^-1),  M_i = H_i P_i^-1 H_i^T,  1e-4 <= w_i <= 1,  sum_i w_i = 1,
 * as f(w) = -log det(sum_i w_i M_i): convex, so the minimiser is one point, found by an active-set Newton iteration in a
 * few steps (fp64, fixed summation order: the same inputs give the same bits on every call; no wall-time limit).  Every
 * covariance is factored once per call (the Kalman stage's blocked Cholesky with the rows of H_i as right-hand sides).
 * What is returned is the MINIMISER, not the iterate NLopt's COBYLA stops at: the reference stops on ftol_abs = 1e-6 of a
 * determinant that is 1e-38 or smaller for filter covariances, i.e. at once.  Two more deliberate deviations:
 *   - the start point is feasible.  The reference starts the k-agent form from w_0 = 1 - k w > 1, w_i = w < 0, which NLopt
 *     rejects, and then falls back to the NEGATIVE weight as a fixed one (ci.cpp:70-73): an indefinite S.  Here the start is
 *     w_i = |w|, w_0 = 1 - k |w| (uniform if that is below 1e-4); pairwise (1 + w, -w) clamped into [1e-4, 1 - 1e-4].
 *   - w = -1 (the reference's default, vio.cpp:191-192) is valid and means "search from no prior"; the result does not
 *     depend on the start.
 * A search that does not converge within 50 steps, or meets a sum_i w_i M_i or a covariance that is not positive definite,
 * returns XK_ESINGULAR (text in xk_last_error); there is no silent fallback to |w| (ci.cpp:70-73,114-116).
 * Limits of a searched entry: m <= 21 rows, at most 8 agents including the own one. */

/* The search alone: k1 (2..8) symmetric positive definite m x m matrices M (host, k1 * m * m doubles, m <= 21), start point
 * w_start (k1 weights >= 1e-4 that sum to one) or NULL = uniform; w (out, k1), *iters (out, may be NULL) = Newton steps taken. */
int xk_ci_solve_weights(xk_handle *h, const double *M, int m, int k1, const double *w_start, double *w, int *iters);
/* The weights of the last searched entry on this handle (also of xk_ci_solve_weights): w (out, 8; own agent first, unused
 * ones zero), *k1 their number, *iters the Newton steps.  All zero before the first search. */
int xk_ci_last_weights(const xk_handle *h, double *w, int *k1, int *iters);
/* The weights the last searched xk_ci_round_device found for its shared track `track`: w (out, 8; own agent first, then the
 * others by rank, unused ones zero), *k1 their number, *iters the Newton steps (both may be NULL).  A track that gave no entry
 * (a gate rejected it) has *k1 = 0 and all weights zero.  XK_EINVAL before the first searched round and for a track index
 * outside the last one.  After a searched round xk_ci_last_weights reports the last fused track's weights. */
int xk_ci_round_weights(const xk_handle *h, int track, double *w, int *k1, int *iters);

/* CovarianceIntersection::fuseCI, k-agent MSCKF form (src/x/ekf/ci.cpp:49-92):
 * S = (1/w0) H P H^T + sum_i (1/w) H_i P_i H_i^T, w0 = 1 - k w,
 * *w_result = 1/w0.  Searched (w < 0): S = sum_i H_i P_i H_i^T / w_i with the searched per-agent weights,
 * *w_result = 1/w_0 (ci.cpp:78-90). */
int xk_fuse_ci_msckf(xk_handle *h, const double *P, int ldp, int n, const double *H, int ldh, int m,
                     int k, const double *const *Ps, const int *ns, const double *const *Hs,
                     double w_other, double *S, int lds, double *w_result);

/* Pairwise SLAM form (ci.cpp:94-127): S = P_a/(1-w) + P_b/w in measurement
 * space, *w_result = 1/(1-w).  Searched (w < 0): the same with w = the searched second weight w_b (ci.cpp:117-122). */
int xk_fuse_ci_slam(xk_handle *h, const double *Pa, int lda, int na, const double *Ha, int ldha,
                    const double *Pb, int ldb, int nb, const double *Hb, int ldhb, int m,
                    double w_other, double *S, int lds, double *w_result);

/* MultiSlamUpdate::processOneMatch (src/x/vio/multi_slam_update.cpp:61-246):
 * 3-row landmark-difference residual between own SLAM feature `feature_id`
 * and the other agent's `o_feature_id`, chi2_3(0.9) gate, pairwise CI, and
 * the 3 diagonal 3x3 blocks of P_j scaled by w_result.  Outputs valid iff
 * *inlier: H (3 x n), res (3), S (3x3), P_j (n x n). */
int xk_multi_slam_match(xk_handle *h, const double *C_q_G, const double *G_p_C, int n_poses,
                        const double *feat, int anchor_idx, int feature_id, const double *P, int ldp,
                        int n, int n_poses_max, const double *o_C_q_G, const double *o_G_p_C,
                        int o_n_poses, const double *o_feat, int o_anchor_idx, int o_feature_id,
                        const double *o_P, int ldop, int no, int o_n_poses_max, double sigma_landmark,
                        double ci_slam_w, int *inlier, double *gamma, double *H, int ldh, double *res,
                        double *S, double *P_j, int ldpj);

/* MSCKF-MSCKF CI block of MsckfUpdate::preProcessOneTrack (src/x/vio/msckf_update.cpp:96-279)
 * for ONE of this agent's tracks that k other agents also observed (k <= 7):
 * joint triangulation over all agents' observations (matched agents first, self last,
 * :113-165), own single-agent gate (:172, :457-463), column-space rows of every agent
 * (:201-203, :439-443), null-space projection of the landmark (:207, :494-501),
 * S_j over all agents (:217-237), chi2(2*sum(L) - 3, 0.95) gate (:243-250), fixed-weight
 * fuseCI (:252-255) and the block scaling of P_j (:256-267).
 *   obs [L x 2], own window lists / P as in xk_stage_*;
 *   per matched agent i: m_obs[i] [m_L[i] x 2], m_q[i] [m_nposes[i] x 4], m_p[i]
 *   [m_nposes[i] x 3] (the lists of its VALID window poses, as for the own agent; its track sees
 *   the LAST m_L[i] of them), m_nposes_max[i] the window size its covariance is laid out for
 *   (m_nposes[i] <= m_nposes_max[i] <= 64: the attitude block of pose p starts at column
 *   15 + 3*m_nposes_max[i] + 3*p, whatever m_nposes[i] is),
 *   m_P[i] [m_n[i] x m_n[i]] dense column-major, m_n[i] = 15 + 6*m_nposes_max[i] + 3*M_i.
 * The joint gate's threshold comes from the table up to 512 degrees of freedom and from the same quantile function
 * beyond (eight agents with windows of 33 and more).
 * Outputs: *self_inlier, *self_gamma; *has_ci; if *has_ci: H (3k x n, ldh), res (3k),
 * S (3k x 3k, lds), P_j (n x n, ldpj), feed them to xk_apply_ci.  H/res/S are defined up to
 * a common orthogonal factor (basis of the null space), H^T S^-1 H and H^T S^-1 res are not. */
int xk_msckf_ci_track(xk_handle *h, const double *obs, int L, const double *C_q_G, const double *G_p_C,
                      int n_poses, const double *P, int ldp, int n, int n_poses_max, double sigma_img, int k,
                      const double *const *m_obs, const int *m_L, const double *const *m_q,
                      const double *const *m_p, const int *m_nposes, const int *m_nposes_max,
                      const double *const *m_P, const int *m_n, double ci_msckf_w, int *self_inlier,
                      double *self_gamma, int *has_ci,
                      double *ci_gamma, double *H, int ldh, double *res, double *S, int lds, double *P_j,
                      int ldpj);

/* ---- MSCKF-SLAM update and persistent-feature initialisation ----
 * Tracks whose landmark becomes a persistent (SLAM) feature this frame (VioUpdater::constructUpdate,
 * vio_updater.cpp:311-321 -> MsckfSlamUpdate, msckf_slam_update.cpp:25-267).  Staged like the MSCKF tracks
 * (CSR of normalised observations, a length-L track sees the last L poses); xk_msckf_build then also builds
 * their null-space rows (stacked between the MSCKF and the SLAM rows, vio_updater.cpp:413-419) and keeps the
 * column-space rows H1, H2, r1 and the triangulated inverse-depth features on the device. */
int xk_stage_msckf_slam(xk_handle *h, const int *trk_off, const double *obs_xy, int K2);
/* After xk_msckf_build: per-track gate result and the MsckfSlamMatrices (types.h) -- H1 (3K2 x n, ldh1),
 * H2 (3K2 x 3K2 block diagonal, ldh2), r1 (3K2), features (3K2); any pointer may be NULL.  H1/H2/r1 are defined
 * up to an orthogonal 3x3 factor per track (basis of the column space); H2^-1 H1, H2^-1 r1, H2^-1 H2^-T are not. */
int xk_msckf_slam_results(xk_handle *h, int *inlier, double *gamma, double *H1, int ldh1, double *H2, int ldh2,
                          double *r1, double *features);
/* StateManager::initMsckfSlamFeatures + addFeatureStates (state_manager.cpp:151-174,199-226) after the update:
 * new_features (out, 3K2) = features - H2^-1 H1 correction + H2^-1 r1, and the covariance blocks of feature
 * slots n_features .. n_features + K2 - 1 of the RESIDENT (posterior) covariance are set to -H2^-1 H1 P (cross)
 * and H2^-1 H1 P (H2^-1 H1)^T + sigma_img^2 H2^-1 H2^-T.  XK_ESINGULAR if an H2 block is singular. */
int xk_init_msckf_slam_features(xk_handle *h, int n_features, const double *correction, double sigma_img,
                                double *new_features);
/* StateManager::initStandardSlamFeatures + addFeatureStates (state_manager.cpp:176-226): k uncorrelated new
 * features in slots n_features.., variances sigma_img^2, sigma_img^2, sigma_rho_0^2 (feature values:
 * SlamUpdate::computeInverseDepthsNew, slam_update.cpp:216-242, stay on the host). */
int xk_init_standard_slam_features(xk_handle *h, int n_features, int k, double sigma_img, double sigma_rho_0);

/* ---- StateManager::manage on the resident covariance (state_manager.cpp:31-149) ----
 * Every covariance operation of manage() -- persistent-feature removal (:52-112), anchor re-parametrisation
 * (reparametrizeFeatures, :351-482), window slide (slideWindow, :484-537) and pose augmentation
 * (augmentCovariance, :273-349) -- is  P <- J P J^T  with a J that is an identity / permutation / zero except
 * for a few 3-row blocks.  The reference forms J densely and does two n^3 products per operation; here J is
 * handed over in CSR (n rows, row_ptr[n+1], 0-based col_idx, val) and applied to the handle's RESIDENT
 * covariance in O(nnz(J)^2 / n + n^2).  host/src/state_manager.cpp builds the J's exactly as the reference. */
int xk_cov_congruence(xk_handle *h, const int *row_ptr, const int *col_idx, const double *val, int nnz);

/* Propagator::propagateCovarianceMatrices (src/x/ekf/propagator.cpp:166-205) on the resident covariance, one
 * IMU step (and, called in a loop, Ekf::repropagateFromStateAtIdx, ekf.cpp:227-252):
 *   P_ii <- F_d P_ii F_d^T + Q_d,  P_iv <- F_d P_iv,  P_vi <- P_vi F_d^T,  P_vv unchanged.
 * f_d, q_d: the 15 x 15 discrete transition and process-noise matrices (column-major, ld >= 15) that
 * Propagator::discreteStateTransition / discreteProcessNoiseCov (:110-164, :207-840) compute on the host. */
int xk_cov_propagate(xk_handle *h, const double *f_d, int ldf, const double *q_d, int ldq);

/* Device-resident CI round (MsckfUpdate::preProcessOneTrack CI block, msckf_update.cpp:96-279, followed by
 * Updater::applyCI per fused entry, updater.cpp:90-93,144-161) against the snapshots of the other agents as they
 * sit in the RCCL receive buffer -- no host staging of the n x n covariances.
 *   d_payloads   DEVICE [world][payload_stride]: xk_pack_payload layout of every agent (own slot unused)
 *   d_tracks     DEVICE [world][n_tracks][1 + 2N]: per shared track the length, then the observations (x,y)
 *   track_len    host [world][n_tracks], n_poses_valid host [world]: the lengths / window sizes found in the above
 *   self_track   host [n_tracks]: index of each shared track among this handle's staged tracks
 * The handle's staged window and its RESIDENT covariance are this agent's side.  Every entry is built from the
 * same prior and applyCI overwrites P each time (the reference's behaviour): on return the resident covariance
 * is the posterior of the last fused entry.  corrections (host, optional): [*n_fused][n].
 * Searched weights (-1 <= ci_msckf_w < 0 with "ci_weight_search" on): per shared track j the weights minimise
 * -log det sum_i w_i M_i^(j), M_i^(j) = H_ij P_i^-1 H_ij^T (m = 3 (world - 1) rows, world matrices; index 0 = own agent, then
 * the others by rank), exactly as xk_msckf_ci_track's searched path.  The two gates are computed before the weights and
 * without them.  Every agent's covariance is factored ONCE per round on the device with the rows of all tracks as right-hand
 * sides; the weights go from the solver to S_ci = sum_i H_i P_i H_i^T / w_i + sigma^2 I and to the scaling of the own pose
 * blocks (1 / w_0) without leaving the device, and reach the host -- with the solver's step counts -- in pinned memory with
 * the gate words: the host still waits once.  A fixed-weight round queues what it always queued.
 *   XK_ESINGULAR   a covariance of ANY agent is not positive definite, whatever the gates say (the text names the agent's
 *                  rank), or the search failed on a track that passes both gates.  Nothing is applied: the resident
 *                  covariance is untouched, *n_fused = 0, the handle keeps working.  A failed search on a track the gates
 *                  reject is ignored.
 * Limit: the FULL n x n covariance of every agent must be positive definite (the reference and the host route invert the full
 * matrix too), so a payload whose unused window slots are zero blocks cannot be searched. */
int xk_ci_round_device(xk_handle *h, const double *d_payloads, long payload_stride, int world, int self_rank,
                       const double *d_tracks, int n_tracks, const int *track_len, const int *n_poses_valid,
                       const int *self_track, double sigma_img, double ci_msckf_w, int *n_fused, double *corrections);

/* ---- inter-agent payload (SimpleState, include/x/ekf/simple_state.h:33-35,
 * assembled at src/x/vio/vio.cpp:447-450) ------------------------------ */

/* Size in doubles of the fixed all-double payload for (N, M): hdr[8] dyn[16]
 * pos[3N] att[4N] feat[3M] anchors[M] cov[n*n]. */
long xk_payload_doubles(int n_poses_max, int n_feat_max);
/* Packs this agent's outgoing payload from the staged window/SLAM state and
 * the CURRENT device-resident P into d_dst (a DEVICE buffer of
 * xk_payload_doubles doubles owned by the caller, e.g. the RCCL send buffer)
 * or, if d_dst is NULL, into a buffer owned by the handle; *d_payload (if
 * non-NULL) receives the device pointer used.  dyn (16) = p,v,q xyzw,b_w,b_a (State::getDynamicStates,
 * state.cpp:87-99) comes from the host. */
int xk_pack_payload(xk_handle *h, double agent_id, double timestamp, const double *dyn16,
                    double *d_dst, double **d_payload);

/* ---- place-recognition request filter + keyframe store ---------------------------
 * The reference answers another agent's request by scoring the request's binary VLAD against its own keyframe
 * database and returning the best keyframe's SimpleState + tracks (VIO::processOtherRequests, vio.cpp:462-496 ->
 * PlaceRecognition::findPlace, place_recognition.cpp:677-683 -> Database::findCandidate, database.cpp:30-49); the
 * requester then matches the returned descriptors against its own (findCorrespondences, place_recognition.cpp:249).
 * The keyframes (payload in xk_pack_payload layout, packed tracks, descriptors, VLAD) stay in device memory, so a
 * response is sent straight from HBM.  Descriptors are rows of desc_bytes bytes (ORB: 32). */
typedef struct xk_pr xk_pr;

/* Vocabulary = a DBoW3 tree (PRVocabulary, types.h:33): k, L, node descriptors [n_nodes][desc_bytes], children
 * [n_nodes][kmax] (-1 padded, in file order), word_of_node [n_nodes] (-1 for inner nodes), node_of_word [n_words].
 * payload_doubles / tracks_doubles: sizes of the per-keyframe device buffers; max_desc: most descriptors per call. */
int xk_pr_create(xk_handle *h, int k, int L, int n_nodes, int kmax, int desc_bytes, const unsigned char *node_desc,
                 const int *children, const int *word_of_node, const int *node_of_word, int n_words,
                 long payload_doubles, long tracks_doubles, int max_desc, xk_pr **out);
void xk_pr_destroy(xk_pr *p);
int xk_pr_vlad_bytes(const xk_pr *p);   /* k^L * desc_bytes (vlad.cpp:27-31: v_length_ / 8) */
int xk_pr_size(const xk_pr *p);         /* keyframes in the store (<= 15, database.h:70) */

/* VLAD::computeVLAD (vlad.cpp:40-66) / Database::computeVLAD (database.cpp:26-28): desc HOST [n][desc_bytes] ->
 * vlad_out HOST [xk_pr_vlad_bytes]. */
int xk_pr_compute_vlad(xk_pr *p, const unsigned char *desc, int n, unsigned char *vlad_out);

/* Database::addKeyframe (database.cpp:51-61): VLAD of the keyframe's descriptors (Keyframe::getDescriptors order:
 * MSCKF, SLAM, OPP tracks, keyframe.cpp:40-52), stored with the DEVICE payload / tracks buffers (copied; may be NULL)
 * and a caller tag; the oldest keyframe is dropped beyond 15. */
int xk_pr_add_keyframe(xk_pr *p, const unsigned char *desc, int n_desc, const double *d_payload, const double *d_tracks,
                       long tag);

/* Database::findCandidate (database.cpp:30-49): best-scoring keyframe with score > pr_score_thr that has not yet
 * been sent to `uav_id` (Keyframe::findOtherUavId); marks it as sent.  *index = position in the store, oldest
 * first, or -1; *score = (v_length - hamming) / v_length of the winner (VLAD::computeScore, vlad.cpp:68-75). */
int xk_pr_find_candidate(xk_pr *p, int uav_id, const unsigned char *query_vlad, double pr_score_thr, int *index,
                         double *score, long *tag);

/* The stored keyframe `index`: DEVICE pointers of its payload / tracks (what VIO::processOtherRequests hands back,
 * vio.cpp:489-495), its descriptor count and tag; desc_out (HOST, optional) receives the descriptors. */
int xk_pr_keyframe(xk_pr *p, int index, const double **d_payload, const double **d_tracks, int *n_desc, long *tag,
                   unsigned char *desc_out);

/* Copies the stored keyframe's payload / tracks into caller-owned DEVICE buffers (e.g. the RCCL send buffer of the
 * response) and waits for the copy. */
int xk_pr_copy_keyframe(xk_pr *p, int index, double *d_payload_dst, double *d_tracks_dst);

/* matcher_->knnMatch(query = received, train = current, k = 2) with NORM_HAMMING (place_recognition.cpp:68-69,249):
 * idx / dist HOST [nq][2], ascending (distance, train index); idx = -1 where the train set is too short. */
int xk_pr_knn_match(xk_pr *p, const unsigned char *query, int nq, const unsigned char *train, int nt, int *idx, int *dist);

/* cv::findEssentialMat(current_points, received_points, K, cv::RANSAC, 0.99, 1.0, mask) of findCorrespondences
 * (place_recognition.cpp:269-281): cur_xy / rec_xy HOST [n][2] float32 pixels of the good matches, in order; mask HOST
 * [n] (1 = inlier), E HOST [9] row-major with rec^T E cur = 0 on normalised coordinates (may be NULL), *n_inliers.
 * n_hyp (1...4096) five-point hypotheses from the counter-based sampler (seed) are ALL evaluated -- the reference's
 * prob = 0.99 only stops a sequential loop early, so it is not a parameter; the winner has the most inliers under the
 * squared Sampson distance <= (threshold_px / ((fx+fy)/2))^2, ties to the lowest hypothesis; no refit.  Three launches
 * on the handle's stream, one synchronisation.  n < 5: XK_OK, *n_inliers = 0, mask and E zeroed (F_1.empty() -> return
 * false); n > max_desc: XK_ECAPACITY; null pointers, fx / fy <= 0, threshold_px < 0, n_hyp out of range: XK_EINVAL. */
int xk_pr_essential_ransac(xk_pr *p, const float *cur_xy, const float *rec_xy, int n, double fx, double fy, double cx,
                           double cy, double threshold_px, int n_hyp, unsigned long seed, unsigned char *mask,
                           double *E /* 9, row-major, may be NULL */, int *n_inliers);

/* What the last xk_pr_essential_ransac (place_recognition.cpp:269-281) left for hypotheses first ... first+count-1:
 * n_cand HOST [count] (0...10 real solutions of the five-point problem), E HOST [count][10][9] (unit Frobenius norm,
 * unused slots zero), inliers HOST [count][10].  Any output may be NULL.  XK_EINVAL outside the last call's range.
 * An inspection path, not part of a frame: it copies straight into the caller's buffers (720 bytes of E per hypothesis, no
 * pinned staging block is kept for it) and waits for the copies once. */
int xk_pr_essential_hypotheses(xk_pr *p, int first, int count, int *n_cand, double *E /* [count][10][9] */,
                               int *inliers /* [count][10] */);

/* PlaceRecognition::findCorrespondences (place_recognition.cpp:137-385, the non-GT_DEBUG branch) in ONE call: what
 * xk_pr_knn_match -> ratio test -> xk_pr_essential_ransac -> mask and duplicate removal -> classification compute as a
 * chain of stage calls and host list work, with nothing returning to the host in between.  One pinned block and one copy
 * in (descriptors and pixels of both sides), six launches on the handle's stream (xk_desc_knn2, xk_corr_candidates,
 * xk_ess_solve, xk_ess_score, xk_ess_mask, xk_corr_finish) with the candidate count in device memory, one result block
 * out, one synchronisation.
 *   2-NN with query = received, train = current; a query passes when its second neighbour exists and
 *   (double)d0 < pr_min_distance && (double)d0 < (double)d1 * pr_ratio_thr (:254-255).  The candidates' pixels, in query
 *   order, go through the essential filter exactly as xk_pr_essential_ransac takes them (same sampler, solver, key and
 *   tie rule: mask and E are bit-equal to that entry on the same pairs).  Then the mask (:275-281), the duplicate search
 *   and the erase loop with its running offset (:283-302; NOT a clean de-duplication, and reproduced as it is), and the
 *   classification (:311-383). */
typedef struct xk_pr_corr_out {
  int status;        /* 0 matched; 1 no current features (:209); 2 no received features (:244); 3 no match passes the
                        distance + ratio test (:265); 4 fewer than 5 candidates or no hypothesis produced a candidate
                        (F_1.empty(), :274); 5 nothing left after mask + duplicate removal (:304) */
  int n_candidates;  /* survivors of the ratio test = pairs given to the RANSAC */
  int n_inliers, winner;
  int n_good;        /* after mask and duplicate removal; 0 unless status == 0 */
  int n_classified;  /* <= n_good (a good match falls in at most one class); 0 unless status == 0 */
  int launches;      /* kernels queued by this call: 6, or 0 for status 1 and 2 (decided on the host) */
  double E[9];       /* as xk_pr_essential_ransac; zero for status 1..4 */
} xk_pr_corr_out;

/* rec_* the received keyframe (query side), cur_* the current features (train side), each HOST in MSCKF | SLAM | OPP
 * order: desc [n][desc_bytes], xy [n][2] float32 pixels.  good HOST [n_rec][2] (queryIdx, trainIdx), classified HOST
 * [n_rec][3] (kind in the numbering of x::MatchKind: 0 MSCKF x OPP, 1 SLAM x SLAM, 2 SLAM x OPP, 3 OPP x OPP; index in
 * the current list of its class; index in the received list of its class); the first n_good / n_classified rows are
 * written; either may be NULL.  For every non-zero status the lists are empty (the reference returns before committing
 * anything).  xk_pr_essential_hypotheses works after this call as after xk_pr_essential_ransac.
 * XK_EINVAL: null pointers, negative counts, class counts beyond their side, fx / fy <= 0, non-finite intrinsics,
 * threshold_px < 0, n_hyp outside 1...4096.  XK_ECAPACITY: n_rec or n_cur above max_desc. */
int xk_pr_find_correspondences(xk_pr *p, const unsigned char *rec_desc, const float *rec_xy, int n_rec,
                               const unsigned char *cur_desc, const float *cur_xy, int n_cur, int n_cur_msckf,
                               int n_cur_slam, int n_rec_msckf, int n_rec_slam, double pr_min_distance, double pr_ratio_thr,
                               double fx, double fy, double cx, double cy, double threshold_px, int n_hyp, unsigned long seed,
                               xk_pr_corr_out *out, int *good /* [n_rec][2], may be NULL */,
                               int *classified /* [n_rec][3], may be NULL */);

/* Inspection of the last xk_pr_find_correspondences: candidates HOST [n_rec][2] (query, train; n_candidates rows written),
 * mask HOST [n_rec] (the essential filter's, zero past the candidates), remove_ids HOST [n_rec] (*n_remove written: the
 * list of :283-296).  Any output may be NULL.  No device work: the rows came back in the call's result block.  XK_EINVAL
 * before a completed call. */
int xk_pr_find_correspondences_stage(xk_pr *p, int *candidates, unsigned char *mask, int *remove_ids, int *n_remove);

/* ---- training a vocabulary (DBoW3::Vocabulary::create, third_party/DBow3/src/Vocabulary.cpp:157-186) -------------
 * Hierarchical k-means of binary descriptors on the device: HKmeansStep (Vocabulary.cpp:233-394) with k-means++ seeding
 * (initiateClustersKMpp, :409-491), Hamming distances, bit-majority means (DescManip::meanValue, DescManip.cpp:26-75) and
 * createWords (:496-515).  The result is bit-defined: the reference's unseeded rand() is replaced by a
 * counter-based sampler on (seed, the node's path in the tree, the seeding step), and the unbounded Lloyd loop by at most
 * max_iter association passes per node.  setNodeWeights is not computed: neither VLAD nor xk_pr_create reads weights.
 * The tree is built level by level on the handle's stream; the host waits once per association pass of a level and once
 * per level, never once per node. */
typedef struct xk_voc xk_voc;

#define XK_VOC_MAX_LEVELS 8
typedef struct {
  int n_nodes, n_words;                 /* sizes of what xk_voc_get returns (n_nodes counts the root) */
  int levels;                           /* levels that had a node to split (<= L) */
  int level_nodes[XK_VOC_MAX_LEVELS];   /* nodes split at each level, trivial ones (n <= k) included */
  int level_passes[XK_VOC_MAX_LEVELS];  /* association passes run at each level = the most any of its nodes needed */
  int capped_nodes;                     /* nodes whose Lloyd loop ended at max_iter, not by convergence */
  int launches, host_waits;             /* kernels queued / stream synchronisations taken by the training */
} xk_voc_outcome;

/* 2 <= k <= 16, 1 <= L <= 8, desc_bytes a multiple of 4 up to 64, k^L * desc_bytes <= 64 MB (as xk_pr_create has it),
 * max_desc >= 1: the most training descriptors.  Otherwise XK_EINVAL (XK_ECAPACITY for the 64 MB bound). */
int xk_voc_create(xk_handle *h, int k, int L, int desc_bytes, int max_desc, xk_voc **out);
void xk_voc_destroy(xk_voc *v);
/* Vocabulary::getFeatures (Vocabulary.cpp:220-228): desc HOST [n][desc_bytes] rows are appended on the device, in call
 * order.  XK_ECAPACITY (nothing appended) beyond max_desc; XK_EINVAL for n < 0 or null rows with n > 0. */
int xk_voc_add(xk_voc *v, const unsigned char *desc, int n);
int xk_voc_count(const xk_voc *v);
int xk_voc_clear(xk_voc *v);            /* forgets the descriptors and the trained tree */
/* HKmeansStep from the root (Vocabulary.cpp:178, :233-394) and createWords (:496-515) on the descriptors added so far.
 * max_iter >= 1.  outcome may be NULL.  No descriptors: XK_OK with only the root (HKmeansStep's early return, :237) --
 * a tree xk_pr_create refuses (n_nodes < 2).  A node with n <= k descriptors gets one child per descriptor (:248-258). */
int xk_voc_train(xk_voc *v, unsigned long seed, int max_iter, xk_voc_outcome *outcome);
/* The trained tree in DBoW3's node order (a node's children are one block of ids, then depth first, :361-393), as
 * xk_pr_create takes it with kmax = k: node_desc HOST [n_nodes][desc_bytes] (root: zeros), children HOST [n_nodes][k]
 * (-1 padded: seeding that stops early and trivial nodes give fewer than k), word_of_node HOST [n_nodes] (-1 for inner
 * nodes and the root), node_of_word HOST [n_words] (the leaves in id order, :505-513).  Any output may be NULL.
 * XK_EINVAL before a training. */
int xk_voc_get(const xk_voc *v, unsigned char *node_desc, int *children, int *word_of_node, int *node_of_word);

/* ---- outlier removal of the tracker's matches (Tracker::track, tracker.cpp:233-293) -----------------------------
 * Every frame the reference undistorts the previous and the current feature list through the FOV model
 * (camera.cpp:62-87,163-168), runs cv::findFundamentalMat(pts1, pts2, cv::RANSAC, 0.3, 0.99, mask) on their float casts
 * and keeps the masked pairs as the frame's matches.  An xk_trk does that on the device of its handle; it needs no
 * vocabulary and no xk_pr.  Intrinsics in pixels (Camera's fx_ ... cy_, camera.cpp:30-33) and the FOV parameter s are
 * fixed at creation (xk_trk_camera_model below gives it another lens); max_matches: most pairs per call. */
typedef struct xk_trk xk_trk;

/* Camera::Camera (camera.cpp:27-48).  max_matches < 1, fx / fy <= 0, non-finite intrinsics: XK_EINVAL. */
int xk_trk_create(xk_handle *h, int max_matches, double fx, double fy, double cx, double cy, double s, xk_trk **out);
void xk_trk_destroy(xk_trk *t);

/* Camera::undistort (camera.cpp:62-87): dist_xy HOST [n][2] distorted pixels -> xy HOST [n][2] undistorted pixels, fp64:
 * r = |((u - cx)/fx, (v - cy)/fy)|, factor tan(r s) / (2 tan(s/2)) / r where r > 0.01 and s != 0, else 1. */
int xk_trk_undistort(xk_trk *t, const double *dist_xy, int n, double *xy);

/* cv::findFundamentalMat(pts1, pts2, cv::RANSAC, threshold_px, 0.99, mask) (tracker.cpp:243-260): prev_xy / cur_xy HOST
 * [n][2] float32 undistorted pixels (the cv::Point2f of :251-256); mask HOST [n] (1 = inlier), F HOST [9] row-major in
 * pixel coordinates with cur^T F prev = 0 and unit Frobenius norm (may be NULL), *n_inliers.  n_hyp (1...4096) seven-point
 * hypotheses from the counter-based sampler (seed) are ALL evaluated -- prob = 0.99 only stops a sequential loop early, so
 * it is not a parameter; the error of a pair is the larger of its two squared point-to-epipolar-line distances in pixels
 * (OpenCV's, not Sampson's), an inlier has error <= threshold_px^2; the winner has the most inliers, ties to the lowest
 * hypothesis; no refit, no degeneracy test of the sample.  Three launches, one synchronisation.  n < 7: XK_OK,
 * *n_inliers = 0, mask and F zeroed (OpenCV returns an empty mask, the loop of :263-268 keeps nothing); n > max_matches:
 * XK_ECAPACITY; null pointers, n < 0, threshold_px < 0, n_hyp out of range: XK_EINVAL. */
int xk_trk_fundamental_ransac(xk_trk *t, const float *prev_xy, const float *cur_xy, int n, double threshold_px, int n_hyp,
                              unsigned long seed, unsigned char *mask, double *F /* 9, row-major, may be NULL */,
                              int *n_inliers);

/* What the last RANSAC of an xk_trk (tracker.cpp:259-260; either entry) left for hypotheses first ... first+count-1:
 * n_cand HOST [count] (0...3 candidates of the seven-point problem), F HOST [count][3][9] (pixel coordinates, unit
 * Frobenius norm, unused slots zero), inliers HOST [count][3].  Any output may be NULL.  XK_EINVAL outside the last call's
 * range;
 * a call with n < 7 ran no hypotheses, so every non-empty range is outside it.  An inspection path, not part of a frame: it copies
 * straight into the caller's buffers. */
int xk_trk_fundamental_hypotheses(xk_trk *t, int first, int count, int *n_cand, double *F /* [count][3][9] */,
                                  int *inliers /* [count][3] */);

/* The per-frame call, tracker.cpp:233-293 whole: prev_dist_xy / cur_dist_xy HOST [n][2] DISTORTED pixels of the tracked
 * pairs (Feature::getXDist / getYDist) -> mask HOST [n], keep_idx HOST [n] (the first *n_inliers entries: the positions
 * of the kept pairs, ascending), prev_xy / cur_xy HOST [n][2] (the first *n_inliers rows: the UNDISTORTED fp64 pixels of
 * the kept pairs in input order, what :262-271 pushes and the matches of :286-293 carry).  The RANSAC sees the float casts
 * of the undistorted pixels, as in xk_trk_fundamental_ransac.  Four launches on the handle's stream, one copy in, one
 * copy out through a pinned block allocated by xk_trk_create, one synchronisation.  Status codes as above; every
 * output pointer is required. */
int xk_trk_filter_matches(xk_trk *t, const double *prev_dist_xy, const double *cur_dist_xy, int n, double threshold_px,
                          int n_hyp, unsigned long seed, unsigned char *mask, int *keep_idx, double *prev_xy, double *cur_xy,
                          int *n_inliers);

/* Tracker's outlier_method_ (tracker.h:56, :256), the method argument of cv::findFundamentalMat: XK_TRK_RANSAC (cv::RANSAC, the
 * default at creation) or XK_TRK_LMEDS (cv::LMEDS); anything else is XK_EINVAL and changes nothing.  Sticky on the object: it
 * governs xk_trk_filter_matches, xk_trk_frame and xk_trk_photo_frame from the next call on.  Under XK_TRK_LMEDS those calls ignore
 * their threshold_px (as OpenCV ignores param1) and keep nothing for n < 8.  It drops no setup and allocates nothing. */
#define XK_TRK_LMEDS 4
#define XK_TRK_RANSAC 8
int xk_trk_outlier_method(xk_trk *t, int method);

/* The lens of the camera, for calibrations the FOV model does not cover (DESIGN 3.10.2 defines the models; they are this project's,
 * not the reference's).  XK_CAM_FOV: 1 coefficient, s -- the same camera as xk_trk_create with that s, bit for bit.  XK_CAM_RADTAN:
 * k1 k2 p1 p2 [k3] (4 or 5 coefficients, k3 = 0 with 4), Kalibr's radtan / OpenCV's plumb-bob model.  XK_CAM_EQUIDISTANT: k1 ... k4,
 * Kannala-Brandt.  All fp64 on conditioned coordinates x = (u - cx)/fx, y = (v - cy)/fy.  Sticky on the object: xk_trk_undistort,
 * xk_trk_distort, xk_trk_filter_matches, xk_trk_frame and xk_trk_photo_frame follow it from the next call on.  It drops no setup and
 * allocates nothing.  An unknown model, a count the model does not take, a non-finite coefficient or a null pointer: XK_EINVAL, and
 * the camera stays what it was.
 * The inverses of the two new models are Newton iterations of at most 20 steps.  A point where the model folds (det J not > 0, or
 * d theta_d / d theta not > 0), whose angle leaves (0, pi/2), or that has not converged after 20 steps is INVALID: its undistorted
 * pixel is its distorted pixel, bit for bit -- finite and inert, never a NaN -- and it is counted (xk_trk_undistort_status). */
#define XK_CAM_FOV 0
#define XK_CAM_RADTAN 1
#define XK_CAM_EQUIDISTANT 2
int xk_trk_camera_model(xk_trk *t, int model, const double *coeffs, int n_coeffs);

/* The forward map of the camera model: xy HOST [n][2] undistorted pixels -> dist_xy HOST [n][2] distorted pixels, fp64.  Capacity and
 * status codes as xk_trk_undistort.  (FOV: r_d = atan(2 r tan(s/2)) / s, the identity where that is not above 0.01.) */
int xk_trk_distort(xk_trk *t, const double *xy, int n, double *dist_xy);

/* What the last xk_trk_undistort, xk_trk_filter_matches, xk_trk_frame or xk_trk_photo_frame (past its first frame, which undistorts
 * nothing) left: *n_invalid, the number of invalid points, and *max_steps, the most Newton steps any point took.  Either may be NULL.
 * Both are 0 under XK_CAM_FOV, and after xk_trk_camera_model.  An inspection path: one small copy and one wait of its own, so a
 * frame's copies and waits are what they were. */
int xk_trk_undistort_status(xk_trk *t, int *n_invalid, int *max_steps);

/* cv::findFundamentalMat(pts1, pts2, cv::LMEDS, ., 0.99, mask), the stage entry beside xk_trk_fundamental_ransac (which stays RANSAC
 * whatever the sticky method is, as this one is LMedS whatever it is): the same inputs, sampler, solver and error, all n_hyp
 * hypotheses evaluated.  Per candidate med = 0.5 (e[(n-1)/2] + e[n/2]) of its ascending errors e, in fp64, a NaN error counting as
 * +inf; a candidate whose median is not finite is not a candidate.  The winner has the smallest median, then the lowest hypothesis,
 * then the lowest candidate.  sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(med), at least 0.001; an inlier has error <= sigma^2.
 * No refit.  *median and *sigma (may be NULL): the winner's.  Three launches, one synchronisation.  n < 8: XK_OK, nothing kept, mask,
 * F, *median and *sigma zeroed.  For 8 <= n <= 13 both middle errors belong to the seven sample points, which every candidate fits
 * exactly: the medians are round-off and the selection arbitrary (in OpenCV too).  Status codes as xk_trk_fundamental_ransac. */
int xk_trk_fundamental_lmeds(xk_trk *t, const float *prev_xy, const float *cur_xy, int n, int n_hyp, unsigned long seed,
                             unsigned char *mask, double *F /* 9, row-major, may be NULL */, int *n_inliers, double *median,
                             double *sigma);

/* What the last call left if it ran LMedS (xk_trk_fundamental_lmeds, or xk_trk_filter_matches or a frame past its first under
 * XK_TRK_LMEDS): median HOST [count][3] of hypotheses first ... first+count-1 (+inf: not a candidate), last HOST [2]: the winner's
 * median and sigma (zeros: no winner).  Either may be NULL.  XK_EINVAL outside that call's range and after any other call that
 * used the scratch.  After an LMedS stage call xk_trk_fundamental_hypotheses returns n_cand and F as usual and zero inliers. */
int xk_trk_fundamental_medians(xk_trk *t, int first, int count, double *median /* [count][3] */, double *last /* [2] */);

/* Caller-supplied models under both criteria: F HOST [m][9] row-major in pixel coordinates, used as given (m = 1...4096), prev_xy /
 * cur_xy HOST [n][2] float32 as above (1 <= n <= max_matches) -> inliers HOST [m] (errors <= threshold_px^2) and median HOST [m]
 * (as defined above; +inf where it is not finite).  For a caller that carries a model over from the previous frame.  It uses the
 * scratch: xk_trk_fundamental_hypotheses and _medians then ask for a filter call first. */
int xk_trk_fundamental_score(xk_trk *t, const float *prev_xy, const float *cur_xy, int n, const double *F /* [m][9] */, int m,
                             double threshold_px, int *inliers /* [m] */, double *median /* [m] */);

/* ---- feature tracking in front of that filter (Tracker::featureTracking, tracker.cpp:623-690) --------------------
 * Every frame the reference runs cv::calcOpticalFlowPyrLK(previous image, current image, pts1, ..., win_size_, max_level_,
 * term_crit_, cv::OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_thr_) on the previous features' distorted pixels and drops every
 * point that failed or left the frame; what is left is the match list xk_trk_filter_matches takes.  The same xk_trk does
 * that on the device.  The algorithm is this project's statement of that call: OpenCV's steps with every
 * integer quantity kept exact -- the sums over the window included -- and fp64 where OpenCV uses float. */

/* The parameters Tracker holds (tracker.h:234-261: win_size_ 31 x 31, max_level_ 2, term_crit_ 30 iterations / eps 0.01,
 * min_eig_thr_ 0.003) and the image size.  Allocates two image slots (pyramid and Scharr derivatives of levels 0 ...
 * levels) on the device and the pinned staging of one image and of the results; calling it again replaces both and
 * forgets the images -- once the new buffers exist: a call that fails (XK_EINVAL, XK_ENOMEM) leaves the earlier setup and
 * its images as they were.  levels is the largest l <= max_level whose size (halved with rounding up, l times) still exceeds
 * the window in both directions, as for every level below it.  XK_EINVAL: width / height outside 16...4096, win_w / win_h
 * outside 3...31 or not smaller than the image, max_level outside 0...4, max_iter outside 1...100, eps outside (0, 10],
 * min_eig_thr < 0. */
int xk_trk_klt_setup(xk_trk *t, int width, int height, int win_w, int win_h, int max_level, int max_iter, double eps,
                     double min_eig_thr);
/* levels of that (the first) set as above, or -1 before xk_trk_klt_setup. */
int xk_trk_klt_levels(xk_trk *t);

/* The second parameter set of a PHOTOMETRIC_CALI build (win_size_photo_, max_level_photo_, min_eig_thr_photo_, vio/types.h:98-106):
 * Tracker::featureTracking uses it from the frame of the first gain estimate on (tracker.cpp:641-651).  Called after
 * xk_trk_klt_setup, with its ranges; max_iter and eps are shared (the reference passes one term_crit_ to both calls).  Its
 * levels follow the rule above with this window.  It is a setup-class call: both image slots are laid out again for the
 * deeper of the two sets' levels (so are the raw slots of a later xk_trk_photo_setup), and every push builds every level up to
 * there; the images are forgotten, every dependent setup is DROPPED and the selection returns to 0, exactly as after a
 * repeated xk_trk_klt_setup.  A call that fails (XK_EINVAL: before xk_trk_klt_setup, a value out of range, a window that does
 * not fit level 0; XK_ENOMEM) leaves the earlier setup, its images and its dependent setups as they were.  A later
 * xk_trk_klt_setup forgets the second set.  An xk_trk that never calls this is, bit for bit and launch for launch, what it
 * was without the entry. */
int xk_trk_klt_second(xk_trk *t, int win_w, int win_h, int max_level, double min_eig_thr);

/* The set that xk_trk_track and both trackings of xk_trk_frame use from now on: sticky, as xk_trk_outlier_method.  It
 * allocates nothing, drops nothing and queues nothing.  The tracking inside xk_trk_photo_calibrate never follows it: it
 * always uses set 0 (tracker.cpp:784-787); xk_trk_photo_frame ignores it and leaves it unchanged (see there).  XK_EINVAL, and
 * the selection as it was: before xk_trk_klt_setup, set 1 without a second set, any value but 0 or 1. */
int xk_trk_klt_select(xk_trk *t, int set);
/* 0 or 1; -1 before xk_trk_klt_setup. */
int xk_trk_klt_selected(xk_trk *t);
/* levels of set 0 or 1; -1 before xk_trk_klt_setup, for a second set that was not declared, for any other value. */
int xk_trk_klt_levels_of(xk_trk *t, int set);

/* previous_img_ = current_img.clone() (tracker.cpp:302) and the new current image: img HOST [height][stride] uint8, stride
 * >= width.  The current slot becomes the previous one; the image is copied (through the pinned staging: the caller's
 * buffer is free on return) and its pyramid and derivatives are queued on the handle's stream -- one launch per level
 * each, no synchronisation but a wait for the previous push's upload.  XK_EINVAL before xk_trk_klt_setup, img NULL,
 * stride < width. */
int xk_trk_push_image(xk_trk *t, const unsigned char *img, int stride);

/* Tracker::featureTracking (tracker.cpp:623-690) from the previous image to the current one: prev_xy HOST [n][2] float32,
 * the cv::Point2f of Feature::getDistPoint2f (:629-633), widened to fp64 -> cur_xy HOST [n][2], status HOST [n] (1 =
 * tracked), min_eig HOST [n] (the err of OPTFLOW_LK_GET_MIN_EIGENVALS: the level-0 minimal eigenvalue per window pixel; 0
 * for a point outside level 0), and the post-filter of :658-686 -- kept iff status != 0 and -0.5 <= x <= width - 0.5,
 * -0.5 <= y <= height - 0.5: keep_idx HOST [n] (the first *n_kept entries, ascending), kept_prev_xy / kept_cur_xy HOST
 * [n][2] (the first *n_kept rows, in input order as the erase loop of :660-686 leaves them).  A non-finite point comes back
 * as it went in with status 0.  One copy in, one launch pair, one copy out, one synchronisation.  Every output is
 * required.  XK_EINVAL: null pointers, n < 0, before xk_trk_klt_setup, fewer than two images pushed; n > max_matches:
 * XK_ECAPACITY; n = 0: XK_OK and *n_kept = 0. */
int xk_trk_track(xk_trk *t, const float *prev_xy, int n, double *cur_xy, unsigned char *status, double *min_eig, int *keep_idx,
                 double *kept_prev_xy, double *kept_cur_xy, int *n_kept);

/* One pyramid level of the previous (which = 0) or the current (1) image as the device holds it (the pyramid that
 * cv::calcOpticalFlowPyrLK builds inside the call of tracker.cpp:648-651): img HOST [h][w] uint8, dIx / dIy HOST [h][w]
 * int16, *w, *h.  Any output may be NULL.  An inspection path, not part of a frame: straight copies.  XK_EINVAL: a level
 * above the deeper of the two sets' levels, an image that has not been pushed. */
int xk_trk_klt_level(xk_trk *t, int which, int level, unsigned char *img, short *dIx, short *dIy, int *w, int *h);

/* ---- detection of the features that are tracked (Tracker::featureDetection, tracker.cpp:390-590) -----------------
 * On the first frame, and again whenever too few features survive (tracker.cpp:160-167, :204-228), the reference runs
 * cv::FAST(img, keypoints, fast_detection_delta_, non_max_supp_) (:441-448), keeps the keypoints inside the border
 * (isFeatureInsideBorder, :536-552), sorts them by score (:483-486) and appends, best first, those that do not lie in
 * the neighbourhood of an old feature or of one appended before (computeNeighborhoodMask :494-534,
 * appendNonNeighborFeatures :564-590).  The same xk_trk does that on the device, on level 0 of an image slot that
 * xk_trk_push_image filled.  The algorithm is this project's statement of those calls; every quantity is an
 * integer and the result is defined bit for bit:
 *   score      s(x, y) = max over the 16 arcs of 9 contiguous circle pixels of the arc's smallest I(circle) - I(x, y), and
 *              of the same with the sign turned, - 1 (OpenCV's cornerScore); a corner has s >= threshold; 3 <= x < W - 3,
 *              3 <= y < H - 3
 *   keypoint   non_max_supp: the corner's s is strictly greater than s at its eight neighbours (0 where no corner)
 *   candidate  margin <= x <= W - margin - 1, margin <= y <= H - margin - 1
 *   order      ascending key ((255 - s) << 24) | (y W + x): score descending, raster order within a score (std::sort
 *              leaves that open)
 *   selection  in that order a candidate is accepted iff no old feature (round half away from zero; a non-finite one
 *              blocks nothing) and no candidate accepted before lies within Chebyshev distance block_half_length of it:
 *              the painted mask with every box clipped to the image, defined also where the reference's unclipped
 *              cv::Rect would assert.
 * Level 0 only (pyramid_depth_ is 1), no descriptors; the intensity a PHOTOMETRIC_CALI build attaches
 * to a detected feature (tracker.cpp:461) is xk_trk_photo_intensity, below. */

/* The parameters Tracker holds (tracker.h:245-255: fast_detection_delta_ 9, non_max_supp_ true, block_half_length_ 20,
 * margin_ 20) and max_candidates (1...32768), the most candidates one image may have.  Called after xk_trk_klt_setup, whose
 * image size it takes; allocates the score image, the key list, the blocked mask and the pinned staging of the result.
 * XK_EINVAL: before xk_trk_klt_setup, threshold outside 1...254, non_max_supp not 0 or 1, block_half_length or margin
 * outside 0...4096, max_candidates outside 1...32768.  A call that fails leaves an earlier detection setup as it was.  A
 * later xk_trk_klt_setup that succeeds DROPS the detection setup with the images: call this again after it. */
int xk_trk_detect_setup(xk_trk *t, int threshold, int non_max_supp, int block_half_length, int margin, int max_candidates);

/* Tracker::featureDetection (tracker.cpp:390-590) on the previous (which = 0) or the current (1) image, as in
 * xk_trk_klt_level -- the reference's re-detection names previous_img_ (:214): old_xy HOST [n_old][2] fp64, the old
 * features' distorted pixels (may be NULL when n_old = 0) -> xy HOST [max_matches][2] (the first *n_found rows: the accepted
 * pixels x, y in ascending key), score HOST [max_matches] (their s), *n_found, *n_candidates (candidates before the
 * selection).  One copy in, three launches, one copy out, one synchronisation.  Every output is required.
 * XK_EINVAL: null outputs, n_old < 0, which not 0 or 1, no detection setup, a slot that has not been pushed.
 * XK_ECAPACITY: n_old > max_matches (both counts 0); more than max_candidates candidates (*n_candidates is the true
 * count, *n_found = 0: nothing was selected); more than max_matches accepted (both counts true).  The lists are then
 * untouched.  Nothing found: XK_OK with *n_found = 0. */
int xk_trk_detect(xk_trk *t, int which, const double *old_xy, int n_old, int *xy, int *score, int *n_found, int *n_candidates);

/* What the last xk_trk_detect left on the device: scores HOST [height][width] uint8, the score image (s at corners, 0
 * elsewhere -- before non-maximum suppression and the border test); keys HOST [max_candidates] (the first *n_candidates
 * entries: the candidates' keys, ascending; not written after a detection that overflowed max_candidates).  Any output
 * may be NULL.  An inspection path, not part of a frame: straight copies.  XK_EINVAL before a detection. */
int xk_trk_detect_stage(xk_trk *t, unsigned char *scores, unsigned int *keys, int *n_candidates);

/* ---- description of the detected features (PlaceRecognition::compute, place_recognition.cpp:72-94) ----------------
 * A MULTI_UAV build describes every FAST keypoint at each detection (tracker.cpp:440-444 -> cv::ORB::compute), hands each
 * feature's descriptor on through the tracking (:675-679) and keeps the whole block as the source of the request's VLAD
 * (descriptros_, place_recognition.cpp:92, :690-692).  The same xk_trk does that on the device, on level 0 of an image slot
 * that xk_trk_push_image filled (cv::FAST keypoints have octave 0).  The algorithm is this project's statement of the call
 * (DESIGN 3.13), defined bit for bit; agreement with OpenCV's own bits is not claimed:
 *   blur       G = the image under the separable taps {18, 34, 49, 54, 49, 34, 18} / 256 (sigma 2), unrounded between the
 *              passes, (sum + 32768) >> 16 once; borders reflect without repeating the edge pixel
 *   filter     a keypoint is kept iff edge <= x < W - edge and edge <= y < H - edge (KeyPointsFilter::runByImageBorder);
 *              kept keypoints keep their input order
 *   direction  (A, B) = 16384 (cos, sin), rounded to integers: of a fixed angle (cv::FAST leaves KeyPoint::angle at -1 and
 *              cv::ORB::compute takes the angle as it finds it: the default, -1 degree), or of the intensity centroid
 *              (m10, m01) of the unblurred image over the disc of radius 15 ((16384, 0) where both moments are 0)
 *   tests      bit i & 7 of byte i >> 3 is G[y + r(x1 B + y1 A)][x + r(x1 A - y1 B)] < the same at (x2, y2) for row i =
 *              (x1, y1, x2, y2) of the pattern; r = division by 16384 rounded half away from zero
 * Level 0 only, WTA_K = 2, no Harris score. */

/* orientation 0: the fixed angle angle_deg; 1: the intensity centroid (angle_deg is ignored but must be finite).  edge
 * (25...4096; OpenCV's edgeThreshold 31).  pattern HOST [256][4] int8, x1 y1 x2 y2 per test, every coordinate within -15
 * ... 15: OpenCV's ORB is the first 256 rows of bit_pattern_31_ in its orb.cpp, which a binding that links OpenCV passes
 * here; NULL selects this project's default, whose descriptors match no vocabulary trained on OpenCV's.
 * (A vocabulary for the default pattern, or for any other descriptor, is trained with xk_voc_* above.)
 * max_desc (1...32768): the most keypoints one call may pass, independent of max_matches.  Called after xk_trk_klt_setup,
 * whose image size it takes; allocates the two blurred images, the result block and its pinned staging.
 * XK_EINVAL: before xk_trk_klt_setup, orientation not 0 or 1, angle_deg not finite, edge or max_desc out of range, a
 * pattern coordinate outside -15...15, a pattern row whose two points coincide.  A call that fails leaves an earlier
 * description setup as it was.  A later xk_trk_klt_setup that succeeds DROPS it with the images: call this again after it. */
int xk_trk_describe_setup(xk_trk *t, int orientation, double angle_deg, int edge, const signed char *pattern, int max_desc);

/* cv::ORB::compute (place_recognition.cpp:83-88) on the previous (which = 0) or the current (1) image: xy HOST [n][2]
 * int32, the keypoints' pixels (any values: the filter decides) -> desc HOST [n][32] (the first *n_kept rows), keep_idx
 * HOST [n] (their positions in xy, ascending), dir HOST [n][2] (A, B of the kept), moments HOST [n][2] (m10, m01 of the
 * kept; zeros with a fixed angle), *n_kept.  The slot's blur is queued by its first description after the push.  One copy
 * in, two launches (three with the blur), one copy out, one synchronisation.  Every output is required.
 * XK_EINVAL: null outputs, n < 0, which not 0 or 1, no description setup, a slot that has not been pushed.
 * XK_ECAPACITY: n > max_desc; the outputs are then untouched.  n = 0 or nothing kept (an image smaller than 2 edge + 1
 * keeps nothing): XK_OK with *n_kept = 0. */
int xk_trk_describe(xk_trk *t, int which, const int *xy, int n, unsigned char *desc, int *keep_idx, int *dir, int *moments, int *n_kept);

/* blurred HOST [height][width] uint8: G of the previous (which = 0) or the current (1) image, computed now if no
 * description of that slot did; pattern HOST [256][4]: the pattern in use, as the device holds it.  Either may be NULL.
 * An inspection path, not part of a frame: straight copies.  XK_EINVAL as for xk_trk_describe. */
int xk_trk_describe_stage(xk_trk *t, int which, unsigned char *blurred, signed char *pattern);

/* ---- Tracker::track in one call (tracker.cpp:134-306) on a feature list that stays on the device ---------------------
 * The stage entries above are the five stages of a frame; xk_trk_frame is the frame: an image goes in, the frame's match
 * list comes out, and previous_features_ (tracker.cpp:299) never leaves the device.  It is Tracker::track of a build WITHOUT
 * PHOTOMETRIC_CALI, on pyramid level 0 as the stage entries are.  Every stage is queued on the handle's
 * stream with its count in device memory; the re-detection is queued on every frame and its kernels return at once
 * where the flag the overflow pass left is clear.  Per frame: one copy of the image in, one copy of the result block out
 * (sized by the host's bound: the resident count plus the detection's packing bound, at most max_matches), and one wait
 * besides the wait for the previous push's staging buffer.
 *
 * The PHOTOMETRIC frame (calibrateImage between the push and the tracking, tracker.cpp:186-190) is an entry of its own,
 * xk_trk_photo_frame below: xk_trk_frame returns XK_EINVAL while a photometric setup is in place on this xk_trk.
 *
 * xk_trk_frame_setup: n_feat_min (tracker.cpp:204), the tile grid of TiledImage (n_tiles_h x n_tiles_w, at most 4096
 * tiles) and max_feat_per_tile (tracker.cpp:614), threshold_px and n_hyp of the outlier removal as in
 * xk_trk_filter_matches.  Called after xk_trk_klt_setup and xk_trk_detect_setup; where an xk_trk_describe_setup is in
 * place every feature carries its descriptor, and the detection's margin must then be at least the description's edge
 * (a detected feature is always described).  XK_EINVAL: before those setups, a parameter out of range, margin < edge.
 * A later xk_trk_klt_setup, xk_trk_detect_setup or xk_trk_describe_setup that succeeds DROPS the frame setup. */
int xk_trk_frame_setup(xk_trk *t, int n_feat_min, int n_tiles_h, int n_tiles_w, int max_feat_per_tile, double threshold_px, int n_hyp);

/* What a frame returns.  The arrays are the caller's, HOST, max_matches rows each; the first n_matches rows are written.
 * prev_xy, cur_xy: undistorted pixels of the match's previous and current feature; prev_dist_xy, cur_dist_xy: their
 * distorted pixels; score: the FAST score the feature was detected with; tiles [.][4]: previous row, previous column,
 * current row, current column as the overflow pass set them (tracker.cpp:598-600) -- for a pair the frame's re-detection
 * added, the previous feature's tile as the detection set it (tracker.cpp:578) and -1, -1, a new Feature's, for the current;
 * origin: the position of the match's feature in the previous frame's match list (in the first frame's detections after
 * a first frame), or -(k + 1) for the k-th feature this frame's re-detection accepted; desc [.][32]: the descriptor
 * (required with a description setup, ignored without). */
typedef struct {
  int n_tracked;       /* pairs the tracking's post-filter kept (tracker.cpp:658-686) */
  int n_left;          /* pairs left by removeOverflowFeatures */
  int redetected;      /* 1: n_left < n_feat_min, the frame re-detected */
  int n_candidates;    /* of the re-detection (of the detection, on a first frame) */
  int n_accepted;      /* features it accepted */
  int n_new_tracked;   /* of those, tracked into the current image */
  int n_matches;       /* pairs the outlier removal kept: the rows written, and the next frame's feature count */
  int winner;          /* its winning hypothesis, -1: none (fewer than 7 pairs, or no candidate) */
  double *prev_xy, *cur_xy, *prev_dist_xy, *cur_dist_xy;
  int *score, *origin, *tiles;
  unsigned char *desc;
} xk_trk_frame_out;

/* One image of Tracker::track: img HOST, height rows of stride bytes.
 * First frame (after the setup, xk_trk_frame_reset, a direct xk_trk_push_image or an XK_ECAPACITY): the image is pushed,
 * featureDetection runs on it with no old features, the accepted features are described and become the resident list in
 * ascending key order; n_candidates and n_accepted are set, n_matches = 0.
 * Every later frame: 1. the push; 2. featureTracking of the resident list (its float cast, tracker.cpp:629-633) and the
 * post-filter; 3. removeOverflowFeatures with its quirks (the last pair is never examined, the counts are those of the
 * current features' tiles and stay as counted); 4. where fewer than n_feat_min pairs are left, featureDetection on the
 * PREVIOUS image outside the neighbourhoods of the previous list, the description, the tracking and post-filter of the
 * new features, appended behind the old pairs -- no second overflow pass; 5. Camera::undistort of both lists and the
 * seven-point RANSAC with n_hyp hypotheses and `seed`, fewer than 7 pairs keep nothing; 6. the kept current features
 * become the resident list.  The result is bit for bit what the stage entries return when chained through the host.
 * XK_EINVAL: null arguments, stride below the width, no frame setup, a photometric setup in place (xk_trk_photo_frame is
 * the frame of that build).
 * XK_ECAPACITY, decided on the device and reported at the frame's wait: more candidates than max_candidates, more
 * features accepted than max_matches, more keypoints than max_desc, old plus new pairs beyond max_matches; the counts
 * reached are returned, n_matches = 0, and the next frame is a first frame.  The stage entries and their inspection
 * entries keep result blocks of their own and work between frames (xk_trk_detect_stage and
 * xk_trk_fundamental_hypotheses then ask for a stage call first: a frame overwrites the scratch they read). */
int xk_trk_frame(xk_trk *t, const unsigned char *img, int stride, unsigned long seed, xk_trk_frame_out *out);

/* The resident list: dist_xy HOST [max_matches][2], score HOST [max_matches], desc HOST [max_matches][32], each may be
 * NULL; *n features (0 before a first frame).  An inspection path: straight copies, one synchronisation. */
int xk_trk_frame_features(xk_trk *t, double *dist_xy, int *score, unsigned char *desc, int *n);

/* The next xk_trk_frame (or xk_trk_photo_frame) is a first frame; the pushed images stay.  XK_EINVAL without a frame setup. */
int xk_trk_frame_reset(xk_trk *t);

/* ---- Tracker::track in one call, a PHOTOMETRIC_CALI build (calibrateImage at tracker.cpp:186-190) -----------------------
 * xk_trk_photo_frame is xk_trk_frame of a build that calibrates every image: the resident list also holds each feature's
 * intensity (Feature::getIntensity), the calibration is fed from it with nothing uploaded, and the frame still has one
 * image copied in, one result block out and one wait.  xk_trk_frame_reset and xk_trk_frame_features serve
 * both frames.  With a second Lucas-Kanade parameter set declared (xk_trk_klt_second) its feature trackings switch to it
 * on the device once the calibration is done, as tracker.cpp:641-651 does (see xk_trk_photo_frame).  It leaves
 * refinePhotometricParams to the caller (xk_trk_photo_gains).
 *
 * xk_trk_photo_frame_setup, after xk_trk_frame_setup AND xk_trk_photo_setup: n_hyp_photo in 1 ... max_hyp of the photo
 * setup caps the gain RANSAC -- a frame with R resident features evaluates max(1, min(R, n_hyp_photo)) hypotheses;
 * threshold_photo is fast_detection_delta_photo_ (tracker.cpp:848), 1 ... 254: the FAST threshold of every detection
 * once a frame has estimated gains (XkPhotoState's done flag, read on the device: the frame of the first estimate
 * already re-detects with it); < 0: no switch.  It allocates the intensities and the larger result block.
 * XK_EINVAL: before either setup, a parameter out of range.  A failed call leaves an earlier setup as it was.  Whatever
 * drops the frame setup drops it, and so does a later xk_trk_photo_setup. */
int xk_trk_photo_frame_setup(xk_trk *t, int n_hyp_photo, int threshold_photo);

/* What a photometric frame returns: the fields of xk_trk_frame_out, the getIntensity() of both features of each match
 * (HOST, max_matches rows each, n_matches written), and the outcome of the frame's calibration with the meaning of the
 * outputs of xk_trk_photo_calibrate: n_cal_kept points its tracking between the raw images kept; estimated, and then
 * a_rel, b_rel, support, frame_ab (otherwise 1, 0, 0 and zeros); done: a frame so far has estimated. */
typedef struct {
  int n_tracked, n_left, redetected, n_candidates, n_accepted, n_new_tracked, n_matches, winner;
  double *prev_xy, *cur_xy, *prev_dist_xy, *cur_dist_xy;
  int *score, *origin, *tiles;
  unsigned char *desc;
  double *prev_intensity, *cur_intensity;
  int n_cal_kept, estimated, done, support;
  double a_rel, b_rel, frame_ab[4];
} xk_trk_photo_frame_out;

/* One image of Tracker::track with PHOTOMETRIC_CALI.
 * First frame: the push (the raw plane, the working plane as its copy), featureDetection on the working plane, the
 * intensity of every accepted feature there at its integer pixel (tracker.cpp:461), the description; no calibration
 * (tracker.cpp:160-168).
 * Every later frame: 1. the push; 2. calibrateImage as xk_trk_photo_calibrate runs it, from the resident points and
 * intensities, with seed_photo: with fewer than 4 resident features only the correction, which corrects iff an earlier
 * frame estimated; the rows of a spatial setup that is still accumulating; 3. featureTracking of the resident list on
 * the WORKING planes; 4. the intensity of the kept current features on the RAW current plane at the truncated pixel
 * (tracker.cpp:666); 5. removeOverflowFeatures; 6. the re-detection on the previous working plane with the threshold
 * selected on the device, the new features' intensities there, their description, tracking, and intensities in the raw
 * current plane; 7. undistortion and the fundamental RANSAC with `seed`; 8. the kept current features and their
 * intensities become the resident list.  Bit for bit what the stage entries return when chained through the host.
 * With a second parameter set (xk_trk_klt_second) the feature trackings of steps 3 and 6 run with set 1 iff XkPhotoState's
 * done flag -- the one the detection's threshold switch reads -- is set when their kernel runs, and with set 0 otherwise: every
 * wavefront reads the flag once and takes one set for its whole feature.  The frame of the first estimate therefore already
 * tracks with set 1 (calibrateImage sets CALIBRATION_DONE at tracker.cpp:849, before the tracking at :193), while the
 * calibration's own tracking in step 2 runs with set 0 (:784-787).  The frame ignores xk_trk_klt_select's selection and leaves it
 * unchanged; after xk_trk_photo_reset it is back on set 0 with no further action.  The switch adds no copy, wait or launch; the
 * chain of stage entries states it as xk_trk_klt_select(done) between xk_trk_photo_calibrate and xk_trk_track.
 * Errors as xk_trk_frame, and XK_EINVAL without the photometric frame setup.  After XK_ECAPACITY the counts and the
 * calibration's outcome are returned (the ring has advanced), and the next frame is a first frame. */
int xk_trk_photo_frame(xk_trk *t, const unsigned char *img, int stride, unsigned long seed, unsigned long seed_photo,
                       xk_trk_photo_frame_out *out);

/* The resident intensities beside xk_trk_frame_features: intensity HOST [max_matches] (may be NULL), *n features.
 * An inspection path: a straight copy, one synchronisation. */
int xk_trk_photo_frame_intensities(xk_trk *t, double *intensity, int *n);

/* ---- photometric calibration of the images (Tracker::calibrateImage, tracker.cpp:761-877; irPhotoCalib.cpp) ---------
 * A PHOTOMETRIC_CALI build passes every frame after the first through calibrateImage (tracker.cpp:186-190) before it is
 * tracked: a Lucas-Kanade pass between the UNCORRECTED images, a box-mean intensity per feature, a RANSAC estimate of the
 * affine gain between the frames chained into a 15-frame history, and a rewrite of every pixel of the current image, which
 * is what featureTracking, featureDetection and PlaceRecognition::compute then see.  The same xk_trk does that on the
 * device.  With a photo setup every image slot has two planes: the RAW one, as pushed, and the WORKING one, which every
 * other xk_trk_* entry reads and which equals the raw one until a correction.  The algorithm is this project's statement
 * of those calls:
 *   intensity  hk = kernel_size / 2; the window of (x, y) is rows y - hk ... y + hk - 1, columns x - hk ... x + hk - 1
 *              (tracker.cpp:866-867), clipped to the image; sum = the EXACT integer sum of its pixels, count their number,
 *              value = (double)sum / (255.0 * (double)count) in fp64, 0 where count is 0 (the reference accumulates
 *              pixel / 255.f in float and divides 0 by 0)
 *   gains      per group: hypothesis h fits four distinct points drawn by the sampler of the RANSAC filters above from
 *              seed + g; the fit is the CLOSED-FORM minimum of the cost of photoetricOptimization.h:57-100 (its 2 x 2 normal
 *              equations by Cramer's rule in fp64) -- the minimum Ceres iterates toward; agreement with Ceres' last iterate
 *              is NOT claimed; a point is an inlier iff |o - (p (a - b) + b)| < 8e-3 (irPhotoCalib.cpp:270-278); most
 *              inliers win, ties to the lowest hypothesis; the refit over the winner's inliers is the same closed form.
 *              ALL n_hyp hypotheses are evaluated (the reference runs as many as the group has points from an unseeded
 *              shuffle).  A group of 4 or fewer points contributes nothing (:116)
 *   chain      irPhotoCalib.cpp:104-160, :212-218 in fp64, operation by operation
 *   correction in float32, every operation rounded once: f = v * (1.f/255.f); c = ((f * (float)(a - b) + (float)b) -
 *              PS[y][x]) * 255.f; x = c truncated toward zero (0 where c is not finite or |c| >= 2^31); m = x % 256 with
 *              C's sign rule; u = max(m, 0); out = u < 128 ? 2u : (u == 128 ? 255 : 512 - 2u) (the table of :42-51)
 * The spatial map PS is estimated on the device too, through the xk_trk_photo_spatial_* entries below; until
 * one is installed the correction takes the caller's map (zeros by default).
 * The second Lucas-Kanade parameter set (tracker.cpp:641-651) is xk_trk_klt_second; the calibration's own tracking always uses the
 * first.  Out of scope: the second FAST threshold through the stage entries (tracker.cpp:848; the caller re-runs the setup --
 * xk_trk_photo_frame switches it on the device), keyframe mode, the detached thread of refinePhotometricParams, pyramid levels above 0. */

/* intensities_kernel_size_ (2...64; tracker.h:366: 30), epsilon_gap and epsilon_base of IRPhotoCalib (finite, in [0, 1]),
 * max_hyp (1...4096): the most hypotheses a gain estimate may evaluate.  Called after xk_trk_klt_setup, whose image size it
 * takes; allocates the raw plane of both slots (images already pushed are copied into it), the spatial map (zeros), the
 * parameter ring (one entry (1, 0), irPhotoCalib.cpp:25), one RANSAC scratch block per group and the pinned staging.  From
 * then on xk_trk_push_image builds the pyramid in the raw plane and copies the slot's block into the working plane, device
 * to device.  XK_EINVAL: before xk_trk_klt_setup, a parameter out of range.  A call that fails leaves an earlier photo
 * setup as it was.  A later xk_trk_klt_setup that succeeds DROPS it with the images: call this again after it. */
int xk_trk_photo_setup(xk_trk *t, int kernel_size, double epsilon_gap, double epsilon_base, int max_hyp);

/* Tracker::computeIntensity (tracker.cpp:860-877) on level 0 of the previous (which = 0) or the current (1) image, its
 * raw (plane = 0) or working (1) plane: xy HOST [n][2] int32 (any values) -> value HOST [n] fp64, sum, count HOST [n]
 * int32.  XK_EINVAL: null pointers, n < 0, which or plane not 0 or 1, no photo setup, a slot that has not been pushed.
 * XK_ECAPACITY: n > max_matches. */
int xk_trk_photo_intensity(xk_trk *t, int which, int plane, const int *xy, int n, double *value, int *sum, int *count);

/* One call of IRPhotoCalib::ProcessCurrentFrame (irPhotoCalib.cpp:95-160, :212-218) with EstimateGainsRansac (:221-312)
 * per group: G groups (1...14), group g = points off[g] ... off[g+1] - 1 (off HOST [G + 1], off[0] = 0, ascending) of
 * o_hist (the intensities in the frame frame_back[g] frames back) and o_cur (in the current frame), both HOST fp64.
 * Calibrate-per-frame passes G = 1, frame_back = {1} (tracker.cpp:832-839); refinePhotometricParams (:698-754) one group
 * per history frame.  -> a_rel, b_rel HOST [G]: each group's refit ((1, 0) for a group of <= 4 points or without an
 * inlier), support HOST [G]: its inlier count, frame_ab HOST [4]: the support-weighted pair relative to the previous frame
 * after the drift adjustments, then the frame's origin pair, which is appended to the ring (the oldest entry is dropped
 * beyond 15).  One copy in, three launches per group and one for the chain, one copy out, one synchronisation.
 * XK_EINVAL: null pointers, G, n_hyp (1...max_hyp) or off out of range, no photo setup, frame_back[g] outside 1 ... the
 * ring's size (the reference would index out of bounds); the ring is then untouched.  XK_ECAPACITY: a group of more than
 * max_matches points. */
int xk_trk_photo_gains(xk_trk *t, int G, const int *off, const double *o_hist, const double *o_cur, const int *frame_back, int n_hyp,
                       unsigned long seed, double *a_rel, double *b_rel, int *support, double *frame_ab);

/* What the last gain estimate (xk_trk_photo_gains or xk_trk_photo_calibrate) left for hypotheses first ... first+count-1
 * of group g: ab HOST [count][2], inliers HOST [count].  Either may be NULL.  Straight copies.  XK_EINVAL outside the last
 * call's range (a group of <= 4 points has no hypotheses). */
int xk_trk_photo_hypotheses(xk_trk *t, int g, int first, int count, double *ab, int *inliers);

/* params_PT_ (irPhotoCalib.cpp:25, :213-218): a, b HOST [15], the ring's pairs, oldest first; *count of them are written. */
int xk_trk_photo_params(xk_trk *t, double *a, double *b, int *count);

/* The ring back to its one entry (1, 0); no gains estimated yet (CALIBRATION_DONE false). */
int xk_trk_photo_reset(xk_trk *t);

/* params_PS_ (irPhotoCalib.cpp:36): ps HOST [height][width] float32, NULL: zeros.  Waits for the upload. */
int xk_trk_photo_set_spatial(xk_trk *t, const float *ps);

/* IRPhotoCalib::getCorrectedImage (irPhotoCalib.cpp:442-472) of the previous (which = 0) or the current (1) image with
 * the ring's last pair: level 0 of the working plane recomputed from level 0 of the RAW plane (so a repeated call gives
 * the same image), then the working plane's pyramid and Scharr derivatives; the slot's blur of xk_trk_describe is redone
 * at the next description.  Queued, no synchronisation.  XK_EINVAL: no photo setup, which not 0 or 1, a slot not pushed. */
int xk_trk_photo_correct(xk_trk *t, int which);

/* img HOST [height][width] uint8: level 0 of a slot's raw plane, the image as pushed.  A straight copy. */
int xk_trk_photo_raw(xk_trk *t, int which, unsigned char *img);

/* Tracker::calibrateImage (tracker.cpp:761-858) whole, between xk_trk_push_image and xk_trk_track (tracker.cpp:186-195):
 *   1. xk_trk_track's two launches from the RAW previous to the RAW current plane on prev_xy (HOST [n][2] float32), with
 *      the post-filter of :803-806
 *   2. the intensities of the kept points on the raw current plane at the truncated pixel (:807-808)
 *   3. the gain estimate with one group, frame_back 1, against the kept rows of prev_intensity (HOST [n] fp64, :810)
 *   4. the correction of the current image
 * -> keep_idx, intensity, sum, count HOST [n] (the first *n_kept rows), a_rel, b_rel, support (one each), frame_ab HOST
 * [4], *estimated.  With n < 4 or fewer than 4 kept points (:763, :795, :826) *estimated = 0, the ring does not advance
 * and the image is corrected (with the ring's last pair) only if an earlier call estimated gains; the gain outputs are
 * then (1, 0), 0 and zeros.  One copy in, one copy out, one synchronisation; the lists stay on the device between the
 * steps.  XK_EINVAL: null pointers, n < 0, n_hyp outside 1...max_hyp, no photo setup, fewer than two images pushed.
 * XK_ECAPACITY: n > max_matches. */
int xk_trk_photo_calibrate(xk_trk *t, const float *prev_xy, const double *prev_intensity, int n, int n_hyp, unsigned long seed,
                           int *keep_idx, double *intensity, int *sum, int *count, int *n_kept, double *a_rel, double *b_rel,
                           int *support, double *frame_ab, int *estimated);

/* ---- the spatial photometric map (IRPhotoCalib, irPhotoCalib.cpp:162-210 and :314-420) ------------------------------
 * PS, the per-pixel map the correction subtracts, comes from IRPhotoCalib itself: every frame it collects correspondences
 * between grid cells, and once enough cells are covered it solves a sparse least-squares problem for one value per cell
 * and smooths the result with a Gaussian-process regression.  Opt-in through xk_trk_photo_spatial_setup: without it no
 * entry above queues a launch more or changes an output.  The algorithm is this project's statement of those lines
 * (DESIGN 3.17), restated in NumPy by tests/photo_spatial_np.py:
 *   grid        cw = width / div, ch = height / div (integer division), cells = cw ch; the cell of pixel (x, y) is
 *               (y / div) cw + x / div.  A point is SKIPPED if one of its pixels lies outside the image, or x / div >= cw,
 *               or y / div >= ch (the remainder column and row of an image that is no multiple of div): the reference
 *               aliases such a pixel into another cell's id or indexes out of bounds there
 *   rows        sequential in point order, group by group (:164-198).  sh = the cell of the history pixel, sc = of the
 *               current one.  Skip if sh == sc or count[sh] > max_count (the reference tests sid_history twice and never
 *               sid_current; restated as written).  Otherwise coverage[sh] = coverage[sc] = 1, the row (sh, sc, b) is
 *               appended, b = o_cur (a_hc - b_hc) - o_hist + b_hc in fp64, every operation rounded once, with (a_hc, b_hc)
 *               = getRelativeGains(ring[last - frame_back], ring[last]) operation by operation (:68-74); then count[sc]
 *               and count[sh] grow by one.  Beyond max_rows a row is dropped and counted in `dropped`; counts and
 *               coverage still advance for it
 *   ready       (double)covered / (double)cells > (double)(float)coverage_thr, strict (:202)
 *   unknowns    the covered cells in ASCENDING CELL ID (the reference numbers them by first appearance: a permutation of
 *               the same unknowns), n of them.  A row reads x[sc] - x[sh] = b.  L = A^T A is the multigraph Laplacian, its
 *               entries exact integers; c = A^T b, each entry summed in ASCENDING ROW ORDER
 *   solve       Jacobi-preconditioned conjugate gradients on L x = c from x = 0, M = diag(L) (a variable of degree 0, all
 *               of whose rows were dropped, keeps x = 0); it stops when |r|^2 < tol^2 |c|^2, tol = 1e-13, or after 2 n
 *               iterations.  In exact arithmetic this is Eigen's preconditioned least-squares CG from zero (:369-379); it
 *               selects the solution with sum deg_i x_i = 0 on every connected component.  Not converging within 2 n
 *               iterations is an outcome, not an error: no map is installed and the accumulation goes on (:372-385)
 *   GP          inputs the cell coordinates (sid % cw, sid / cw), outputs x; K_ij = sf^2 exp(-d^2 / (2 l^2)) + sn^2 [i = j]
 *               in fp64 from the FLOAT values of the hyperparameters (defaults 5, 0.01, 0.01, :53-55); K alpha = x by the
 *               same iteration, tolerance and cap.  The reference factors K in float (LDLT): agreement with its last bits
 *               is NOT claimed
 *   prediction  coarse[r][c] = (float) sum_i K((c, r), X_i) alpha_i over every cell; PS[y][x] = coarse[min(y / div, ch - 1)]
 *               [min(x / div, cw - 1)] (the clamp replaces the reference's out-of-bounds read on an image that is no
 *               multiple of div)
 * The estimate runs on the caller's thread (the reference starts a std::thread, :204).  Out of scope: keyframe mode, the
 * reference's first-appearance variable order, the float LDLT's rounding. */

/* What an estimate did: n unknowns, the iterations and final relative residual |r| / |rhs| of both solves, converged
 * (both of them). */
typedef struct {
  int n, converged;
  int ls_iterations, gp_iterations;
  double ls_residual, gp_residual;
} xk_photo_spatial_outcome;

/* div (2...256: temporal_params_div), coverage_thr (spatial_params_thr, kept as a float), max_count (SP_max_correscount_:
 * 500), max_rows (the row list's capacity) and the GP's length scale, sigma_f, sigma_n (kept as floats, each > 0).  Called
 * after xk_trk_photo_setup.  Allocates counts, coverage, the row list, two dense n_max x n_max fp64 matrices with n_max =
 * min(cells, 2048), vectors and a pinned status block.  XK_EINVAL: no photo setup, div out of range, fewer than 2 cells,
 * a parameter that is not finite, max_count < 1, max_rows < 1, a hyperparameter <= 0.  A call that fails leaves an earlier
 * spatial setup as it was.  A later xk_trk_klt_setup or xk_trk_photo_setup DROPS it. */
int xk_trk_photo_spatial_setup(xk_trk *t, int div, double coverage_thr, int max_count, int max_rows, double gp_length,
                               double gp_sigma_f, double gp_sigma_n);

/* One ProcessCurrentFrame worth of rows against the ring as it stands (call it after xk_trk_photo_gains): G groups as in
 * xk_trk_photo_gains, pix_hist, pix_cur HOST [off[G]][2] int32 (x, y), o_hist, o_cur HOST [off[G]] fp64.  One copy in, one
 * launch of one wavefront, the status through pinned memory.  After an installed estimate it does nothing (XK_OK).
 * XK_EINVAL: null pointers, G or off out of range, no spatial setup, frame_back[g] outside 1 ... ring size - 1.
 * XK_ECAPACITY: a group of more than max_matches points.
 * xk_trk_photo_calibrate, with a spatial setup that is still accumulating and on a frame that estimated gains, queues the
 * same kernel behind its chain on lists it already holds on the device (the truncated prev_xy of the kept points, their
 * truncated current pixels, previous and new intensities; one group, frame_back 1): no extra copy, no extra
 * synchronisation, and every output of that call stays as it is. */
int xk_trk_photo_spatial_add(xk_trk *t, int G, const int *off, const int *pix_hist, const int *pix_cur, const double *o_hist,
                             const double *o_cur, const int *frame_back);

/* Where the accumulation stands: rows kept, cells covered, cells, ready (above), rows dropped, state (0 accumulating,
 * 1 estimated: a map is installed and accumulation has stopped, 2 the last estimate did not converge and accumulation
 * goes on).  Any pointer may be NULL.  One small copy and a wait. */
int xk_trk_photo_spatial_status(xk_trk *t, int *rows, int *covered, int *cells, int *ready, int *dropped, int *state);

/* Rows first ... first+count-1: sid_hist, sid_cur HOST [count] int32, b HOST [count] fp64; counts HOST [cells] int32,
 * coverage HOST [cells] uint8.  Straight copies, any pointer may be NULL.  XK_EINVAL: a range outside the kept rows. */
int xk_trk_photo_spatial_rows(xk_trk *t, int first, int count, int *sid_hist, int *sid_cur, double *b, int *counts,
                              unsigned char *coverage);

/* EstimateSpatialParameters on the rows accumulated so far: numbering, L and c, the least squares, the GP, the prediction
 * and the upsample, all on the device; the host reads a done flag through pinned memory after every batch of 32
 * iterations, and every such wait has a bound (XK_EDEVICE beyond it).  install = 1 and convergence: the map is copied into
 * the PS plane, device to device, and accumulation stops.  No convergence: XK_OK, outcome->converged = 0, nothing is
 * installed, state 2.  XK_EINVAL: no spatial setup, null outcome, no row accumulated.  XK_ECAPACITY: n > n_max. */
int xk_trk_photo_spatial_estimate(xk_trk *t, int install, xk_photo_spatial_outcome *outcome);

/* The last estimate's intermediates, for tests: var_of_cell HOST [cells] int32 (-1: not covered), L HOST [n][n], c, x,
 * alpha HOST [n] fp64, coarse HOST [cells] float32, ps HOST [height][width] float32 (coarse and ps only after an estimate
 * that converged).  Straight copies, any pointer may be NULL.  XK_EINVAL: no estimate since the setup or the last reset. */
int xk_trk_photo_spatial_stage(xk_trk *t, int *var_of_cell, double *L, double *c, double *x, double *alpha, float *coarse, float *ps);

/* Counts, coverage and rows back to empty, the state back to accumulating.  The PS plane keeps what it holds. */
int xk_trk_photo_spatial_reset(xk_trk *t);

/* ---- the track manager's candidate tracks: normalisation and baseline check ----------------------------------------
 * TrackManager::manageTracks (src/x/vio/track_manager.cpp:115-436) sorts a frame's matches into persistent (SLAM) and
 * opportunistic tracks; its numerical part is Camera::normalize(track, max_size) and checkBaseline (:576-636) of every
 * track that may become a measurement.  Neither depends on the state of the list walk, so the same xk_trk does both for
 * all of a frame's candidates in one call (the walk itself is host/src/track_manager.cpp). */

/* Capacities of one xk_trk_baseline call: at most max_tracks tracks with max_obs observations in all.  Allocates the
 * device block and its pinned mirror; a call that fails leaves an earlier setup as it was.  XK_EINVAL: max_tracks or
 * max_obs < 1 (or beyond 2^20 / 2^26). */
int xk_trk_baseline_setup(xk_trk *t, int max_tracks, int max_obs);

/* K tracks in CSR form: trk_off HOST [K+1] (in observations, ascending), obs_xy HOST [trk_off[K]][2] fp64 UNDISTORTED
 * PIXELS oldest first, drop_last HOST [K]; C_q_G HOST [n_quats][4] (x,y,z,w), the window's camera attitudes oldest
 * first.  Track k is checked against the first n_quats - drop_last[k] attitudes (drop_last = 1: the reference's
 * cam_rots_short, for tracks that ended at the previous frame) and cropped to its newest min(length, that list's size)
 * observations.
 * -> norm_off HOST [K+1], norm_xy HOST [norm_off[K]][2]: the kept observations as (u - cx) / fx, (v - cy) / fy with the
 *    intrinsics of xk_trk_create, equal to x::Camera::normalize bit for bit;
 *    delta_xy HOST [K][2]: per axis, max - min over the kept rays (x, y, 1) rotated into the list's last camera
 *    (both quaternions normalised, Cn_q_Ci = conj(Ci_q_G) Cn_q_G, ray = conj(Cn_q_Ci) (0,x,y,1) Cn_q_Ci, divided by
 *    its z) AND the unrotated last observation, where the reference starts.  A NaN coordinate takes no part, an
 *    infinite one does; a NaN last observation gives NaN;
 *    flag HOST [K]: delta_x > min_baseline_x_n || delta_y > min_baseline_y_n.
 * One wavefront per track; one copy in, one launch, one copy out, one synchronisation.  K = 0 is XK_OK.
 * XK_EINVAL: null pointers, K < 0, before xk_trk_baseline_setup, trk_off not ascending, a track of fewer than 2
 * observations, drop_last beyond 1, n_quats outside 2...64, n_quats - drop_last < 2 (the cropped length would be), K
 * or trk_off[K] beyond the capacities.  The object stays usable after every one of them. */
int xk_trk_baseline(xk_trk *t, const int *trk_off, const double *obs_xy, const unsigned char *drop_last, int K,
                    const double *C_q_G, int n_quats, double min_baseline_x_n, double min_baseline_y_n, int *norm_off,
                    double *norm_xy, double *delta_xy, unsigned char *flag);

/* ---- TrackManager::manageTracks on the device: the tracks stay there from frame to frame ----
 * The whole of manageTracks (track_manager.cpp:115-436) in one call per frame: the association of the matches with the
 * persistent tracks, the rebuild of the opportunistic ones, the baseline batch, the dead-track pass, the promotion walk
 * with its tile rule and the MSCKF-SLAM / standard split (csrc/xk_track_store.hip.h).  The result equals
 * x::TrackManager's (host/src/track_manager.cpp) and tests/track_manager_np.py's: ids, order, lengths, lost indices and
 * every coordinate bit for bit.  Each of the max_tracks slots keeps a track's newest 64 observations, its true length
 * and its id; the id counter starts at 1 and goes on across frames and across xk_trk_tracks_clear. */

/* The five measurement lists of a call, in the order xk_trk_tracks_out::n_list counts them */
#define XK_TRACKS_MSCKF 0          /* over-long opportunistic tracks whose baseline passes */
#define XK_TRACKS_MSCKF_SHORT 1    /* dead opportunistic tracks */
#define XK_TRACKS_NEW_SLAM_STD 2   /* new persistent tracks, standard initialisation */
#define XK_TRACKS_NEW_MSCKF_SLAM 3 /* new persistent tracks, MSCKF-SLAM initialisation */
#define XK_TRACKS_PERSISTENT 4     /* the persistent tracks cropped to their newest min(n_poses_max, 64) observations */
/* xk_trk_tracks_out::status */
#define XK_TRACKS_OUTSIDE_GRID 1   /* a match's current feature lies outside the tile grid: XK_EINVAL */
#define XK_TRACKS_CAPACITY 2       /* more candidate or live tracks than max_tracks: XK_ECAPACITY */
#define XK_TRACKS_BOOKKEEPING 3    /* the walk found the fullest tile without a track ("tile bookkeeping out of step"): XK_EDEVICE */

/* What a manage call returns.  The caller sets the three capacities and the five pointers; the call fills the rest.
 * lost_slam_idxs [cap_lost]: TrackManager::getLostSlamTrackIndexes, the lost persistent tracks' indices before the
 * frame's deletions.  claimed: 1 where a persistent track took the match (manageTracks erases those from its list); it has no
 * capacity field: it must hold n bytes for xk_trk_tracks_manage and, for xk_trk_tracks_manage_frame, the n_matches of the frame it
 * is fed from (xk_trk_create's max_matches always suffices).
 * The five lists lie behind one another in list order as one CSR: ids [cap_entries], off [cap_entries + 1] in
 * observations, xy [cap_obs][2] the normalised coordinates (u - cx) / fx, (v - cy) / fy of Camera::normalize, oldest
 * first; list l is the n_list[l] entries behind those of the lists before it.
 * Capacities a call needs, with P persistent plus new persistent and O opportunistic tracks in the store before it:
 * cap_lost >= P, cap_entries >= O + n + P, cap_obs >= (O + n) * n_quats + P * min(n_poses_max, 64). */
typedef struct xk_trk_tracks_out {
  int status;                    /* 0, XK_TRACKS_OUTSIDE_GRID, XK_TRACKS_CAPACITY, XK_TRACKS_BOOKKEEPING */
  int n_persistent, n_new_persistent, n_opportunistic;   /* the store's own lists after the call */
  int n_lost, n_claimed, n_candidates, n_candidate_obs;  /* candidates: tracks of the call's baseline batch */
  long long next_id;             /* the id the next started track gets */
  int n_list[5];
  int cap_lost, cap_entries, cap_obs;
  int *lost_slam_idxs;
  unsigned char *claimed;
  long long *ids;
  int *off;
  double *xy;
} xk_trk_tracks_out;

/* Allocates the store for max_tracks tracks, the result block and its pinned mirror.  The tile grid is TiledImage's of
 * a width x height image (tiled_image.cpp:98-105); min_baseline_*_n and multi_uav as TrackManager's constructor takes
 * them; the intrinsics are xk_trk_create's, the most matches of a call its max_matches.  A later successful setup
 * replaces the store (empty, ids from 1); a failed one leaves the earlier one as it was.
 * XK_EINVAL: max_tracks outside 1...2^20, tile counts below 1 or more than 4096 tiles, width or height below 1, a
 * threshold that is NaN, multi_uav other than 0 or 1.  XK_ENOMEM: the allocation failed.
 * Cost.  max_tracks is a capacity, not a working size: three steps of a manage call run in ONE workgroup or wavefront and grow with
 * the lists, not with the device -- the stable sort of n opportunistic tracks (n^2 / 1024 comparisons per thread), the in-order
 * resolve of a frame with contested claims (one step of three barriers per item) and the promotion walk (one step per opportunistic
 * track).  They are measured at a few hundred tracks (0.31 ms at 400); at tens of thousands of live tracks a call
 * takes seconds.  Every loop is bounded all the same. */
int xk_trk_tracks_setup(xk_trk *t, int max_tracks, int n_tiles_h, int n_tiles_w, int width, int height,
                        double min_baseline_x_n, double min_baseline_y_n, int multi_uav);

/* manageTracks of n matches given as HOST columns in the layout of xk_trk_frame_out: prev_xy, cur_xy (undistorted
 * pixels), prev_dist_xy, cur_dist_xy [n][2] fp64, score [n] (both features of a match carry it).  A feature's tile is
 * computed from its distorted pixels.  C_q_G HOST [n_quats][4] (x,y,z,w), the window's camera attitudes oldest first.
 * opp_ids / n_opp_ids: the caller's list of setOppUpgradesMSCKF (multi_uav: required, may be empty); the call consumes
 * it: *n_opp_ids is 0 on XK_OK.  May be NULL single-agent.
 * One copy in, four launches, one copy out, one wait.
 * XK_EINVAL: before xk_trk_tracks_setup; n outside 0...max_matches; a null column with n > 0; C_q_G null or n_quats
 * outside 3...64; n_poses_max < 3; n_slam_features_max < 0; min_track_length outside 1...n_poses_max; opp_ids null with
 * *n_opp_ids > 0, *n_opp_ids outside 0...max_tracks, n_opp_ids null with multi_uav; a null output pointer or a capacity
 * below the bound above; a match outside the tile grid (status XK_TRACKS_OUTSIDE_GRID).
 * XK_ECAPACITY (status XK_TRACKS_CAPACITY): O + (min_track_length <= 2 ? n : 0) > max_tracks, or the frame starts
 * more tracks than there are free slots (the frame's dead tracks hold theirs until the call ends).
 * The two refusals with a status are decided on the device before anything changes and reported at the call's wait:
 * the store, the id counter and *n_opp_ids are what they were.  The object stays usable after every one of these errors.
 * XK_EDEVICE: a HIP error; status XK_TRACKS_BOOKKEEPING (which a consistent store cannot produce); or counts in the result block
 * that fail the host's range checks.  Only after XK_EDEVICE has the store already been modified, and the host's copy of the list
 * lengths (which bound later calls' capacities and the removal indices) is stale: call xk_trk_tracks_clear, or set the store up
 * anew, before the next frame. */
int xk_trk_tracks_manage(xk_trk *t, const double *prev_xy, const double *cur_xy, const double *prev_dist_xy,
                         const double *cur_dist_xy, const int *score, int n, const double *C_q_G, int n_quats,
                         int n_poses_max, int n_slam_features_max, int min_track_length, long long *opp_ids,
                         int *n_opp_ids, xk_trk_tracks_out *out);

/* The same on the matches the last xk_trk_frame / xk_trk_photo_frame of this xk_trk left in its result block on the
 * device: only the attitudes and the ids go up.  A first frame is a valid empty match list.
 * XK_EINVAL as xk_trk_tracks_manage, and: without a frame setup, before a frame, after xk_trk_frame_reset, after a
 * frame that returned an error. */
int xk_trk_tracks_manage_frame(xk_trk *t, const double *C_q_G, int n_quats, int n_poses_max, int n_slam_features_max,
                               int min_track_length, long long *opp_ids, int *n_opp_ids, xk_trk_tracks_out *out);

/* One of the store's own lists: which = 0 persistent, 1 new persistent, 2 opportunistic.  *n: its length; per track
 * ids [*n], lengths [*n] (true lengths), obs [*n][64][4] (undistorted x, y, distorted x, y; the newest min(length, 64)
 * observations oldest first, the rows behind them zero), score [*n][64], tiles [*n][64][2] (row, column).  Any array
 * may be NULL.  An inspection path: a gather and straight copies.  XK_EINVAL: before xk_trk_tracks_setup, which outside
 * 0...2, n null. */
int xk_trk_tracks_lists(xk_trk *t, int which, long long *ids, int *lengths, double *obs, int *score, int *tiles, int *n);

/* TrackManager::removePersistentTracksAtIndex, removeNewPersistentTracksAtIndexes (idxs HOST [n] in strictly increasing
 * order) and clear (the id counter stays).  Tiny launches on the handle's stream with no wait of their own.
 * XK_EINVAL: before xk_trk_tracks_setup; an index at or beyond the list's length as the last result block and the
 * removals since give it; idxs null with n > 0, n < 0, indices not increasing.  Nothing is removed then. */
int xk_trk_tracks_remove_persistent(xk_trk *t, unsigned int idx);
int xk_trk_tracks_remove_new_persistent(xk_trk *t, const unsigned int *idxs, int n);
int xk_trk_tracks_clear(xk_trk *t);

/* xk_msckf_build + xk_qr_compress queued on the handle's stream with NO host synchronisation and no host outputs:
 * together with the non-blocking staging calls and xk_cov_congruence / xk_cov_propagate, a whole frame -- covariance
 * propagation, StateManager::manage, per-feature build, QR compression, Kalman update -- is queued back to back and
 * xk_apply_update's single synchronisation brings the correction, the status and the gate results back.
 * For callers that have something between constructUpdate and applyUpdate that rewrites the covariance -- the applyCI entries of
 * the MULTI_UAV order (updater.cpp:84-97).  [T_H | z] does not depend on the covariance once the gates have read the prior (the
 * per-feature kernel, queued here), so where the single launch can take the Kalman update along (narrow systems, n <= 206) the
 * compression itself is queued by xk_apply_update, behind those entries, with the update inside: one launch there instead of one
 * here and five there.  xk_qr_compress / xk_fetch_flags behave as before: an xk_qr_compress between this call and xk_apply_update
 * runs the compression then and there, and xk_apply_update applies the [T_H | z] it left (no second compression).  No STAGING call
 * (xk_stage_*, xk_msckf_build) may come between the two: it would replace the rows the deferred compression is to read. */
int xk_build_compress_async(xk_handle *h, double sigma_img);

/* xk_build_compress_async with the Kalman update of Updater::applyUpdate(correction_total = 0, cov_update = true)
 * (updater.cpp:117-141) queued as well: inside the compression launch where the geometry allows it (windows of up to 31 poses
 * without persistent features: the update is applied block by block as the panels of the QR complete and costs the launch
 * ~5 us), behind it otherwise.  xk_apply_update(h, NULL, 1, correction) then only waits for the result; any other
 * correction_total / cov_update there is XK_EINVAL.  For the single-agent order with iekf_iter = 1 (updater.cpp:99-110); NOT for
 * the MULTI_UAV order, whose applyCI entries replace the covariance between constructUpdate and applyUpdate (:84-97). */
int xk_build_compress_update_async(xk_handle *h, double sigma_img);

/* The same for ONE PASS of the iterated update (updater.cpp:99-110, iekf_iter > 1): both arguments of the applyUpdate that
 * follows are known when constructUpdate is called -- correction_total is what the passes so far accumulated (:140), cov_update is
 * "this is the last pass" -- so the pass is queued whole: corr = K (res + H corr_total) - corr_total (:126-128), the covariance
 * updated only if cov_update.  corr_total: n doubles on the host, NULL = zeros.  xk_apply_update(h, the same corr_total, the same
 * cov_update, correction) then only waits; other arguments there are XK_EINVAL and leave the queued pass collectable. */
int xk_build_compress_update_pass_async(xk_handle *h, double sigma_img, const double *corr_total, int cov_update);
/* The gate results of the last build (any pointer may be NULL); synchronises the stream if it is still busy. */
int xk_fetch_flags(xk_handle *h, int *inlier_msckf, double *gamma_msckf, int *inlier_slam, double *gamma_slam);

/* ---- range-facet and sun-angle rows (VioUpdater::constructUpdate, vio_updater.cpp:352-423) ----
 * Staged like the visual inputs and consumed by the next build (xk_msckf_build, xk_build_compress*_async, xk_visual_update_staged): the
 * reference uses a measurement once (timestamp = -1, :380, :402), so a build with nothing newly staged has no such rows; xk_run_steps /
 * xk_bench_staged replay the staged update with them in every step, as do the retries of an update.  The rows never go through the QR:
 * they are appended as built to whatever system the update applies ([T; H_aux]^T [T; H_aux] is the Gram matrix of the whole stack).
 * Their variances follow the reference's stack: it compresses when its rows -- 2 L - 3 per MSCKF / MSCKF-SLAM track, 2 M, 1 range, 2 sun,
 * gated out or not -- exceed n + 1, and then weighs EVERY row with sigma_img^2 (vio_updater.cpp:487-509: a compressed range row counts as
 * if sigma_range were sigma_img, a reference quirk kept on purpose); uncompressed, each row keeps its own variance. */

/* RangeUpdate::processRangedFacet (src/x/vio/range_update.cpp:61-270) as stacked at vio_updater.cpp:358-382: one row, the LRF range
 * against the plane of the facet of SLAM features facet[3] (indices into the staged features: TrackManager::featureTriangleAtPoint, host
 * code of the mirror's x::TrackManager; the camera model that gives the undistorted normalised image point (img_x_n, img_y_n) of the ray,
 * vio.cpp:289-294), gated by chi2_1(0.9) against the prior: a rejected row stays as a zero row of variance 1.  Preconditions of the
 * reference (range.timestamp > 0.1, a SLAM track, a facet found) are the caller's.  XK_EINVAL: no SLAM features staged, an id outside
 * [0, M) or repeated, sigma_range <= 0. */
int xk_stage_range(xk_handle *h, double range, double img_x_n, double img_y_n, const int facet[3], double sigma_range);
/* SolarUpdate::processSunAngle (src/x/vio/solar_update.cpp:36-94) as stacked at vio_updater.cpp:386-405: two rows over the IMU attitude
 * error (columns 6..8) from the IMU attitude q_xyzw (state.getOrientation()) and the sensor's x / y angles in degrees.
 * calib: 8 doubles S_q_I (w, x, y, z), G_sun (x, y, z; normalised here), var_sun (deg^2); NULL = the reference's constants
 * (solar_update.cpp:47-56, marked "TODO import from param file" there: a real sensor needs its own values). */
int xk_stage_sun_angle(xk_handle *h, const double q_xyzw[4], double x_angle_deg, double y_angle_deg, const double *calib);
/* Range gate of the last build (range_update.cpp:246-262): *range_inlier = 1 / 0, or -1 if it had no range row; *range_gamma. */
int xk_fetch_aux_flags(xk_handle *h, int *range_inlier, double *range_gamma);
/* The rows of the last build as built (h_lrf then h_sns, vio_updater.cpp:407-421): *rows (0..3), H (rows x n, ldh >= 3, column-major),
 * res (rows), r_diag (rows: the variances the update gives them) -- for a host that runs xk_apply_update_dense on the stack itself. */
int xk_aux_rows(xk_handle *h, double *H, int ldh, double *res, double *r_diag, int *rows);

/* Updater::applyCI (updater.cpp:144-161) on the RESIDENT covariance: P <- sym((I - K H) ci_P), K = ci_P H^T S^-1,
 * replaces the handle's covariance and stays on the device; only the n-vector correction comes back.  A compressed
 * [T_H | z] waiting for xk_apply_update is left alone, so the reference's order -- constructUpdate, the applyCI loop,
 * then applyUpdate on the post-CI covariance (updater.cpp:84-97) -- needs no covariance transfer. */
int xk_apply_ci_resident(xk_handle *h, const double *ci_P, int ldc, int n, const double *H, int ldh, int m,
                         const double *res, const double *S, int lds, double *correction);

/* Save (restore = 0) / bring back (restore = 1) a device-side copy of the resident covariance; 2 / 3: the same on a second slot,
 * which the filter loop (x::Ekf with a resident covariance) keeps for itself: the prior of an update that the IMU thread may lap
 * (Ekf::repropagateFromStateAtIdx, ekf.cpp:229-239, discards such an update). */
int xk_snapshot_P(xk_handle *h, int restore);

/* ---- measurement ----------------------------------------------------- */

#define XK_NSTAGE 6
/* stage order: 0 msckf_feature, 1 slam_rows, 2 caqr_panel0 (first per-tile panel launch), 3 caqr_rest,
 * 4 kalman_update, 5 unused */
typedef struct {
  float total_ms;               /* one staged update, HIP events on the handle's stream */
  float stage_ms[XK_NSTAGE];    /* per update, summed over the stage's launches */
  int stage_launches[XK_NSTAGE];
  char stage_name[XK_NSTAGE][32];
  int n, c1, k_tracks, rows_stacked, n_leaf, n_levels;
} xk_timing;

/* Runs `steps` staged visual updates back to back on the handle's stream
 * (each from the same staged prior; results of the last one stay resident)
 * and reports HIP-event timings averaged per update. */
int xk_bench_staged(xk_handle *h, double sigma_img, int warmup, int steps, xk_timing *out);

/* Enqueues `steps` sequential staged visual updates (same staged prior, the
 * posterior of the last one left in the handle's output buffer) and waits for
 * them; nothing crosses PCIe.  This is the timed region of bench.py. */
int xk_run_steps(xk_handle *h, double sigma_img, int steps);

/* Which schedule compressed the last update -- 0 the multi-launch CAQR, 2 the pipelined single launch (1 was round 2's
 * register-resident kernel, no longer built: the value is never reported), 3 the multi-launch CAQR for the first panels of a tall system (windows of 34..64
 * poses) and one or two single launches for its last <= 192 columns, 4 no compression at all: the stack was the SLAM features' rows alone
 * (2 M rows against n > 3 M columns) or a small stack whose nominal rows are at most n -- the reference compresses only when rows >
 * columns, vio_updater.cpp:487, and neither does this: the rows go to the update as built -- or the update had no track and no SLAM
 * feature at all (nothing to compress) -- whether the single-launch path is armed for the next update, how many launches have given up on
 * this handle so far (workgroups not co-resident: another process on the GPU, a CU mask) and the reason code of the last one
 * (2 XCD-local hand-off, 3 uneven XCD placement, 4 / 5 / 6 waiting for the last level / the roots / the tiles, 8 the Kalman role
 * waiting for rows of R, 9 more rows passed the gates than the tiles of the launch hold -- not a co-residency problem: the fast
 * path stays armed for smaller stacks).  A launch that
 * gives up costs one bounded retry (<= 2 ms) and the update is redone by the multi-launch schedule with the same result; the
 * handle tries the fast path again after "caqr_rearm" (64) clean updates, doubling that distance at every further give-up.
 * xk_last_error() carries the same information as text.  Any pointer may be NULL. */
int xk_caqr_status(const xk_handle *h, int *schedule, int *armed, int *giveups, int *last_reason);

/* Operational switches of the compression on a live handle.  "caqr_resident": 0 = the multi-launch schedule serves every update
 * (e.g. a GPU this process knowingly shares), 1 (default) = the single launch where the shape allows it; "caqr_rearm": clean
 * multi-launch updates after which a single-launch path that gave up is tried again (default 64, doubling at every further give-up);
 * "caqr_tail": 0 = tall systems (windows of 34..64 poses) are factored by the multi-launch schedule to the last panel, 1 (default) = their
 * last <= 192 columns by one or two single launches, 2 = their last <= 96 columns by one; "slam_split": 1 (default) = systems with SLAM
 * features and more than 206 error states compress only the tracks' rows, in the pose columns, and append the features' own rows to the
 * compressed system as built, and a stack of SLAM rows alone or of at most n nominal rows goes to the update uncompressed (same posterior;
 * xk_qr_compress keeps returning the whole stack's upper-triangular T_H), 0 = the whole stack is compressed every time.
 * Unknown name: XK_EINVAL.  The release library reads nothing from the environment; the experiment switches, test hooks, debug
 * exports and probe kernels of the lab build are declared in xk_lab.h.  No counterpart in the reference. */
int xk_set_option(xk_handle *h, const char *name, int value);

#ifdef __cplusplus
}
#endif
#endif /* XK_H_ */
