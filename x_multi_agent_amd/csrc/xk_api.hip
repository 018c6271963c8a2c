// xk_api.hip -- C ABI (include/xk.h) of the MI355X-native xVIO EKF-update engine.
// Host-side orchestration only: every number in a result is produced by the
// HIP kernels in xk_feature.hip.h / xk_linalg.hip.h / xk_ci.hip.h.
#include "../../include/xk.h"
#ifdef XK_LAB
#include "../../include/xk_lab.h"
#endif

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "xk_chi2_table.h"
#include "xk_chi2_quantile.h"
#include "xk_feature.hip.h"
#include "xk_slaminit.hip.h"
#include "xk_linalg.hip.h"
#include "xk_caqr_pipe.hip.h"
#include "xk_ci.hip.h"
#include "xk_ciw.hip.h"
#include "xk_ciw_round.hip.h"
#include "xk_aux.hip.h"

#define XK_VERSION_NUM 201

#include "xk_handle.hip.h"

extern "C" const char *xk_strerror(int s) {
  switch (s) {
    case XK_OK: return "ok";
    case XK_EINVAL: return "invalid argument";
    case XK_ESINGULAR: return "innovation covariance not positive definite";
    case XK_ENAN: return "non-finite value";
    case XK_EDEVICE: return "HIP runtime error";
    case XK_ENOMEM: return "out of memory";
    case XK_ECAPACITY: return "problem exceeds handle capacity";
  }
  return "unknown status";
}
extern "C" const char *xk_last_error(const xk_handle *h) { return h ? h->err : "null handle"; }
extern "C" int xk_version(void) { return XK_VERSION_NUM; }
extern "C" void *xk_stream(xk_handle *h) { return h ? (void *)h->stream : nullptr; }

static int create_impl(int device, int n_poses_max, int n_feat_max, int k_max, xk_handle **out);
extern "C" int xk_destroy(xk_handle *h);
// (a failure part-way through releases everything allocated so far)

extern "C" int xk_create(int device, int n_poses_max, int n_feat_max, int k_max, xk_handle **out) {
  if (!out) return XK_EINVAL;
  *out = nullptr;
  xk_handle *h = nullptr;
  const int rc = create_impl(device, n_poses_max, n_feat_max, k_max, &h);
  if (rc != XK_OK) { if (h) xk_destroy(h); return rc; }
  *out = h;
  return XK_OK;
}

static int create_impl(int device, int n_poses_max, int n_feat_max, int k_max, xk_handle **out) {
  if ( n_poses_max < 2 || n_poses_max > 64 || n_feat_max < 0 || k_max < 0) return XK_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return XK_EDEVICE;
  if (device < 0 || device >= ndev) return XK_EINVAL;
  xk_handle *h = (xk_handle *)calloc(1, sizeof(xk_handle));
  if (!h) return XK_ENOMEM;
  *out = h;   // the caller destroys it if anything below fails
  h->device = device;
  h->N = n_poses_max;
  h->Mmax = n_feat_max;
  h->Kmax = k_max;
  h->n = XK_CORE + 6 * n_poses_max + 3 * n_feat_max;
  h->na = h->n - XK_CORE;
  h->C1 = h->na + 1;
  h->C1P = round_up(h->C1, 64);
  if (h->C1P > 512) return XK_ECAPACITY;
  const int dmax = 2 * n_poses_max - 3;
  h->DB = dmax <= 64 ? 64 : 128;   // rows per tile slot (one track per tile; SLAM rows are packed DB per tile)
  const int slam_tiles = (2 * n_feat_max + h->DB - 1) / h->DB;
  h->ntiles_max = k_max + n_feat_max + slam_tiles;   // MSCKF tracks, MSCKF-SLAM tracks, packed SLAM rows
  h->CM = round_up(h->n + 1 + 3, 16);   // (+ 3: the range-facet and sun-angle rows appended to an uncompressed stack of n rows)
  h->LDA = h->CM + round_up(h->n + 1, 16);
  HIPCHK(h, hipSetDevice(device));
  HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  HIPCHK(h, hipEventCreateWithFlags(&h->ev_flags, hipEventDisableTiming));
  HIPCHK(h, hipEventCreateWithFlags(&h->ev_flags_done, hipEventDisableTiming));
  for (auto &e : h->ev) HIPCHK(h, hipEventCreate(&e));
  const size_t nn = (size_t)h->n * h->n;
  h->obs_cap = (size_t)k_max * n_poses_max;
  // window lists in one allocation, observations + track offsets in another: a staging call is ONE host-to-device copy
  // (small copies run as copy kernels of ~5 us each on the update's critical path)
  HIPCHK(h, dalloc(&h->d_q, 7 * (size_t)n_poses_max));
  HIPCHK(h, hipMalloc((void **)&h->d_done_cnt, sizeof(unsigned)));
  HIPCHK(h, hipMemset(h->d_done_cnt, 0, sizeof(unsigned)));
  h->h_win = (double *)calloc(7 * (size_t)n_poses_max, sizeof(double));
  if (!h->h_win) return fail(h, XK_EDEVICE, "host allocation");
  h->upd.ct = (double *)calloc((size_t)h->n, sizeof(double));   // correction_total of a queued pass (XkPending)
  if (!h->upd.ct) return fail(h, XK_ENOMEM, "host allocation");
  h->d_p = h->d_q + 4 * (size_t)n_poses_max;
  HIPCHK(h, dalloc(&h->d_obs, 2 * h->obs_cap + ((size_t)k_max + 2) / 2 + 1));
  h->d_trk_off = (int *)(h->d_obs + 2 * h->obs_cap);
  HIPCHK(h, dalloc(&h->d_feat, 3 * (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_zlast, 2 * (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_anchor, (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_chi_s, (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_P, nn));
  HIPCHK(h, dalloc(&h->d_Pout, nn));
  HIPCHK(h, dalloc(&h->d_fq, (size_t)450));
  HIPCHK(h, dalloc(&h->d_chi95, (size_t)XK_CHI2_LEN));
  HIPCHK(h, hipMemcpy(h->d_chi95, XK_CHI2_095, sizeof(double) * XK_CHI2_LEN, hipMemcpyHostToDevice));
  // (+ 256 rows behind the slots: where the first of two tail launches leaves its R for the second one, XkCaqrPipeArgs::extra_row0 --
  //  zero outside the trapezoid the launch writes, like d_R)
  HIPCHK(h, dalloc(&h->d_A, ((size_t)h->ntiles_max * h->DB + 256) * h->C1P));
  HIPCHK(h, hipMemset(h->d_A + (size_t)h->ntiles_max * h->DB * h->C1P, 0, sizeof(double) * 256 * h->C1P));
  h->hc_stride = xk_hc_stride(h->DB, h->C1P);
  h->opt_hlite = env_int("XK_HLITE", 1);
  h->opt_gate_form = 1;
  h->rows_compact = false;
  HIPCHK(h, dalloc(&h->d_Hc, (size_t)std::max(k_max, 1) * h->hc_stride));
  HIPCHK(h, dalloc(&h->d_tile_rows, (size_t)h->ntiles_max));
  for (auto &pp : h->d_panel) HIPCHK(h, dalloc(&pp, (size_t)(h->ntiles_max + 10) * 256));
  HIPCHK(h, dalloc(&h->d_inl, (size_t)k_max));
  HIPCHK(h, dalloc(&h->d_inl_s, (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_gn, (size_t)k_max));
  HIPCHK(h, dalloc(&h->d_gam, (size_t)k_max));
  HIPCHK(h, dalloc(&h->d_gam_s, (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_gpf, 3 * (size_t)k_max));
  HIPCHK(h, dalloc(&h->d_R, (size_t)h->C1P * h->C1P));
  HIPCHK(h, hipMemset(h->d_R, 0, sizeof(double) * (size_t)h->C1P * h->C1P));
  // (d_R2: the measurement systems that are NOT the upper-triangular R of the whole stack -- split compression, uncompressed stacks;
  //  sized for C1P rows, and CM <= C1P + 16 rows of an uncompressed stack fit because its rows are at most n)
  HIPCHK(h, dalloc(&h->d_R2, (size_t)(h->C1P + 32) * h->C1P));
  HIPCHK(h, hipMemset(h->d_R2, 0, sizeof(double) * (size_t)(h->C1P + 32) * h->C1P));
  {
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, device));
    h->n_cu = prop.multiProcessorCount;
    // The single-launch schedules need all 256 workgroups co-resident, one per CU.  Decide what can be decided up front:
    // the device must expose 256 CUs to this process (SPX mode, no CU mask visible in the properties) and the runtime must
    // agree that a 768-thread workgroup of each kernel fits a CU; what cannot be known here (another process on the GPU,
    // a CU mask set behind the runtime's back) is caught by the placement census and the bounded spins inside the launch.
    h->persist_ok = h->DB == 64 && h->C1 <= XkPipeWide::COLS && h->n_cu == 256;
    if (h->persist_ok) {
      int nb1 = 0;
      const void *kfn = h->C1 <= XkPipeNarrow::COLS ? (const void *)xk_caqr_pipe<XkPipeNarrow> : (const void *)xk_caqr_pipe<XkPipeWide>;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb1, kfn, XK_PIPE_THREADS, 0) != hipSuccess) nb1 = 0;
      h->persist_ok = nb1 >= 1;
      if (h->persist_ok && h->C1 <= XkPipeNarrow::COLS) {
        int nb2 = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb2, (const void *)xk_caqr_pipe<XkPipeNarrow2>, XK_PIPE_THREADS, 0) != hipSuccess) nb2 = 0;
        if (nb2 < 1) h->opt_split = -1;      // (that geometry's kernel does not fit a CU: never taken)
      }
      (void)hipGetLastError();
    }
    h->fast_capable = h->persist_ok;
    h->tail_capable = h->DB == 128 && h->n_cu == 256 && h->C1 > 32;
    if (h->tail_capable) {
      int nbt = 0, nbt4 = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbt, (const void *)xk_caqr_pipe<XkPipeTail>, XK_PIPE_THREADS, 0) != hipSuccess) nbt = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbt4, (const void *)xk_caqr_pipe<XkPipeTail4>, XK_PIPE_THREADS, 0) != hipSuccess) nbt4 = 0;
      h->tail_capable = nbt >= 1 && nbt4 >= 1;
      (void)hipGetLastError();
    }
    h->tail_ok = h->tail_capable;
    h->opt_tail = env_int("XK_CAQR_TAIL", 1);
    h->opt_slam_split = env_int("XK_SLAM_SPLIT", 1);
    h->opt_pipe_min_rows = env_int("XK_PIPE_MIN_ROWS", 1);   // (512 until round 6: smaller stacks went to the multi-launch schedule -- 23 launches, 0.45 ms against 0.32)
    h->rearm_after = env_int("XK_CAQR_REARM", 64);
    h->opt_resident = env_int("XK_CAQR_RESIDENT", 1);
    h->opt_poison = env_int("XK_CAQR_RESIDENT_POISON", 0);
    h->opt_test_stall = env_int("XK_CAQR_TEST_STALL", 0);
    h->opt_tall26 = env_int("XK_CAQR_TALL26", 1);
    h->opt_kalman = env_int("XK_PIPE_KALMAN", 1);
    if (h->opt_split >= 0) h->opt_split = env_int("XK_PIPE_SPLIT", 1);   // (-1: the 152-tile kernel does not fit a CU on this device -- stays off)
    if (!h->fast_capable && h->DB == 64 && h->C1 <= XkPipeWide::COLS) {
      // Say so once, where an operator sees it: every update of this handle takes the multi-launch schedule (~1.6x slower).
      snprintf(h->err, sizeof(h->err), "single-launch CAQR unavailable on device %d: %s; the multi-launch schedule serves every update",
               device, h->n_cu != 256 ? "the process does not see 256 compute units (partition mode or CU mask)"
                                      : "a 768-thread workgroup of the kernel does not fit a compute unit");
      static const int quiet = env_int("XK_QUIET", 0);
      if (!quiet) fprintf(stderr, "xk: %s (n_cu = %d)\n", h->err, h->n_cu);
    }
    if (h->persist_ok || h->tail_capable) {
      // cross-XCD slabs of the single launch, TWO sets (a launch works on one and re-arms the other for its successor with the
      // NOT-YET pattern of the data-polled hand-offs, xk_xcd_sync.hip.h): per set X1 | X2 ([panels][16 strips][16 x C1P]) | X1P
      // (the tail launch of a tall system runs the last XkPipeTail::COLS / 16 panels only)
      const size_t np = h->persist_ok ? (size_t)(h->C1 + 15) / 16 : (size_t)XkPipeTail4::COLS / 16, strips = np * XK_PIPE_RLS;
      h->xslab_doubles = strips * 16 * h->C1P * 2 + strips * 256;
      HIPCHK(h, dalloc(&h->d_x1, 2 * h->xslab_doubles));
      HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->d_x1, (int)(XK_NOTYET_BITS & 0xffffffffu), 2 * 2 * h->xslab_doubles, h->stream));
      HIPCHK(h, dalloc(&h->d_rs, (size_t)8 * XK_PIPE_NT_MAX * 16 * h->C1P));
      HIPCHK(h, dalloc(&h->d_rpb, (size_t)8 * XK_PIPE_NT_MAX * 256));
      HIPCHK(h, dalloc(&h->d_xsync, (size_t)2 * XP_WORDS * 16));
      HIPCHK(h, hipMemset(h->d_xsync, 0, sizeof(unsigned) * 2 * XP_WORDS * 16));
      h->xsync_phase = 0;
#ifdef XK_LAB
      HIPCHK(h, dalloc(&h->d_pdbg, (size_t)XK_PDBG_WORDS));
      HIPCHK(h, hipMemset(h->d_pdbg, 0, sizeof(long long) * XK_PDBG_WORDS));
#endif
    }
  }
  HIPCHK(h, dalloc(&h->d_Maug, (size_t)h->CM * h->LDA));
  HIPCHK(h, dalloc(&h->d_X, (size_t)h->CM * h->LDA));
  HIPCHK(h, dalloc(&h->d_corr, (size_t)h->n + 4));   // + the status words right behind it: one copy brings both back
  HIPCHK(h, dalloc(&h->d_ct, (size_t)h->n));
  HIPCHK(h, dalloc(&h->d_tmpH, (size_t)h->CM * h->n));
  HIPCHK(h, dalloc(&h->d_tmpS, (size_t)h->CM * h->CM));
  HIPCHK(h, dalloc(&h->d_tmpP, nn));
  HIPCHK(h, dalloc(&h->d_rdiag, (size_t)h->CM));
  HIPCHK(h, dalloc(&h->d_tmpz, (size_t)h->CM));
  HIPCHK(h, dalloc(&h->d_aux, 3 * ((size_t)h->n + 1) + 8));
  HIPCHK(h, dalloc(&h->d_Taug, (size_t)h->CM * ((size_t)h->n + 2)));
  // The status words and the correction of the resident path (xk_apply_update) are written by the kernels straight into
  // pinned host memory through its device-visible address: after the stream synchronisation that ends an update the host
  // reads them in place -- no device-to-host copy (a ~4 us blit kernel plus its launch gap at the end of every frame).
  HIPCHK(h, hipHostMalloc((void **)&h->h_out, sizeof(double) * ((size_t)h->n + 4), hipHostMallocDefault));
  memset(h->h_out, 0, sizeof(double) * ((size_t)h->n + 4));
  h->d_status = (int *)(h->h_out + h->n);
  HIPCHK(h, dalloc(&h->d_payload, (size_t)xk_payload_doubles(n_poses_max, n_feat_max)));
  HIPCHK(h, dalloc(&h->d_ci, (size_t)4 * nn + 64 * (size_t)h->n + 1024));
  HIPCHK(h, dalloc(&h->d_ciw, (size_t)XK_CIW_WS));
  h->h_pin_doubles = nn + 8 * (size_t)h->n + 4 * (size_t)k_max + 4 * (size_t)n_feat_max + 1024;
  HIPCHK(h, hipHostMalloc((void **)&h->h_pin, sizeof(double) * h->h_pin_doubles));
  h->csr_cap = 24 * (size_t)h->n + 3 * (size_t)n_feat_max * h->n;
  {
    const size_t m = (size_t)std::max(n_feat_max, 1);
    HIPCHK(h, dalloc(&h->d_trk2_off, m + 1));
    HIPCHK(h, dalloc(&h->d_inl2, m));
    HIPCHK(h, dalloc(&h->d_gn2, m));
    HIPCHK(h, dalloc(&h->d_obs2, 2 * m * n_poses_max));
    HIPCHK(h, dalloc(&h->d_gpf2, 3 * m));
    HIPCHK(h, dalloc(&h->d_W2, m * h->DB * h->na));
    HIPCHK(h, dalloc(&h->d_gam2, m));
    HIPCHK(h, dalloc(&h->d_H1, 3 * m * h->n));
    HIPCHK(h, dalloc(&h->d_H2, 9 * m));
    HIPCHK(h, dalloc(&h->d_r1, 3 * m));
    HIPCHK(h, dalloc(&h->d_feat2, 3 * m));
    h->h_trk2_off = (int *)calloc(m + 1, sizeof(int));
    if (!h->h_trk2_off) return fail(h, XK_ENOMEM, "host track offsets");
  }
  HIPCHK(h, dalloc(&h->d_csr_v, h->csr_cap + XK_CORE * XK_CORE + 9 * (size_t)n_feat_max * n_feat_max + 7 * (size_t)n_poses_max + ((size_t)h->n + 2 + h->csr_cap) / 2 + 1));
  h->d_csr_i = nullptr;   // (the integer part follows the values of each operand)
  h->h_trk_off = (int *)calloc((size_t)k_max + 1, sizeof(int));
  if (!h->h_trk_off) return fail(h, XK_ENOMEM, "host track offsets");
  HIPCHK(h, hipHostMalloc((void **)&h->h_pin_i, sizeof(int) * ((size_t)k_max + n_feat_max + 512)));
  h->stage_bytes = std::max({sizeof(double) * 2 * h->obs_cap + sizeof(int) * ((size_t)k_max + 1), sizeof(double) * 7 * (size_t)n_poses_max,
                             (sizeof(int) + sizeof(double)) * h->csr_cap + sizeof(int) * ((size_t)h->n + 1) + sizeof(double) * (XK_CORE * XK_CORE + 9 * (size_t)n_feat_max * n_feat_max + 7 * (size_t)n_poses_max),
                             sizeof(double) * 8 * (size_t)std::max(n_feat_max, 1)}) + 256;
  for (auto &sp : h->h_stage) HIPCHK(h, hipHostMalloc((void **)&sp, h->stage_bytes));

  HIPCHK(h, hipHostMalloc((void **)&h->h_flag_i, sizeof(int) * ((size_t)k_max + n_feat_max + 8)));
  HIPCHK(h, hipHostMalloc((void **)&h->h_flag_d, sizeof(double) * ((size_t)k_max + n_feat_max + 8)));
  memset(h->d_status, 0, sizeof(int) * 4);
  HIPCHK(h, hipMemset(h->d_tile_rows, 0, sizeof(int) * (size_t)h->ntiles_max));
  h->sigma_img = 0.0;
  *out = h;
  return XK_OK;
}

extern "C" int xk_destroy(xk_handle *h) {
  if (!h) return XK_OK;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  void *ptrs[] = {h->d_q, h->d_obs, h->d_feat, h->d_zlast, h->d_anchor, h->d_chi_s,
                  h->d_P, h->d_Pout, h->d_chi95, h->d_A, h->d_tile_rows, h->d_panel[0], h->d_panel[1], h->d_inl, h->d_inl_s,
                  h->d_gn, h->d_gam, h->d_gam_s, h->d_gpf, h->d_R, h->d_Maug, h->d_X, h->d_corr,
                  h->d_ct, h->d_tmpH, h->d_tmpS, h->d_tmpP, h->d_rdiag, h->d_tmpz, h->d_payload,
                  h->d_ci};
  for (void *p : ptrs)
    if (p) hipFree(p);
  for (void *p2 : {(void *)h->d_trk2_off, (void *)h->d_inl2, (void *)h->d_gn2, (void *)h->d_obs2, (void *)h->d_gpf2, (void *)h->d_W2,
                   (void *)h->d_gam2, (void *)h->d_H1, (void *)h->d_H2, (void *)h->d_r1, (void *)h->d_feat2})
    if (p2) hipFree(p2);
  free(h->h_trk2_off);
  if (h->d_csr_v) hipFree(h->d_csr_v);
  if (h->d_Hc) hipFree(h->d_Hc);
  if (h->d_R2) hipFree(h->d_R2);
  if (h->d_aux) hipFree(h->d_aux);
  if (h->d_Taug) hipFree(h->d_Taug);
  free(h->upd.ct);
  if (h->d_Psnap) hipFree(h->d_Psnap);
  if (h->d_Psnap2) hipFree(h->d_Psnap2);
  if (h->d_fq) hipFree(h->d_fq);
  for (void *p4 : {(void *)h->d_rs, (void *)h->d_rpb, (void *)h->d_xsync})
    if (p4) hipFree(p4);
  for (void *p3 : {(void *)h->d_x1, (void *)h->d_pdbg})
    if (p3) hipFree(p3);
  if (h->d_ciws) hipFree(h->d_ciws);
  if (h->d_ciw) hipFree(h->d_ciw);
  if (h->d_ciwr) hipFree(h->d_ciwr);
  if (h->d_batch) hipFree(h->d_batch);
  if (h->h_batch) hipHostFree(h->h_batch);
  if (h->h_ci_w) hipHostFree(h->h_ci_w);
  free(h->h_trk_off);
  if (h->h_out) hipHostFree(h->h_out);
  free(h->h_win);
  if (h->d_done_cnt) hipFree(h->d_done_cnt);
  if (h->h_pin) hipHostFree(h->h_pin);
  if (h->h_pin_i) hipHostFree(h->h_pin_i);
  for (auto &sp : h->h_stage)
    if (sp) hipHostFree(sp);

  if (h->h_flag_i) hipHostFree(h->h_flag_i);
  if (h->h_flag_d) hipHostFree(h->h_flag_d);
  for (auto &e : h->ev)
    if (e) hipEventDestroy(e);
  if (h->copy_stream) { hipStreamSynchronize(h->copy_stream); hipStreamDestroy(h->copy_stream); }
  for (int j = 1; j < 8; ++j) {
    if (h->ci_stream[j]) { hipStreamSynchronize(h->ci_stream[j]); hipStreamDestroy(h->ci_stream[j]); }
    if (h->ci_join[j]) hipEventDestroy(h->ci_join[j]);
  }
  if (h->ci_fork) hipEventDestroy(h->ci_fork);
  if (h->ev_flags) hipEventDestroy(h->ev_flags);
  if (h->ev_flags_done) hipEventDestroy(h->ev_flags_done);
  if (h->stream) hipStreamDestroy(h->stream);
  free(h);
  return XK_OK;
}

// ---------------------------------------------------------------------------
// staging
// ---------------------------------------------------------------------------
// next slot of the pinned ring: host inputs are copied there and go to the device with an asynchronous copy, so that
// staging never waits for the device (the caller's buffers are free on return, as before)
// A slot is reused XK_STAGE_SLOTS staging calls later.  Nothing in between need have synchronised the stream (a loop of
// xk_cov_congruence, repeated re-staging), and the copy that reads a slot may still be queued.  The handle counts the slots
// handed out since it last KNEW its stream to be idle (every update ends with a synchronisation: xk_apply_update,
// read_status); when the ring is about to wrap without one, it synchronises itself.  In a filter loop that never happens --
// a frame uses five or six slots -- so staging costs no event and no wait there.
static void stage_stream_idle(xk_handle *h) { h->stage_since_sync = 0; }
static char *stage_slot(xk_handle *h, size_t bytes) {
  if (bytes > h->stage_bytes) return nullptr;
  if (++h->stage_since_sync >= XK_STAGE_SLOTS) {
    // about to wrap onto a slot whose copy may still be queued: wait; if the wait itself fails the slot is not handed out
    if (hipStreamSynchronize(h->stream) != hipSuccess) { --h->stage_since_sync; return nullptr; }
    h->stage_since_sync = 1;
  }
  const int s = h->stage_next;
  h->stage_next = (s + 1) % XK_STAGE_SLOTS;
  return h->h_stage[s];
}

// The completion markers kernels write into pinned host memory behind their results (xk_apply_update has the whole story).
// XK_SPIN_DONE=0 (lab build): no marker is asked for, the stream's completion signal is waited for instead.
static int spin_done() { static const int on = env_int("XK_SPIN_DONE", 1); return on; }
static unsigned long long *done_marker(xk_handle *h) { return reinterpret_cast<unsigned long long *>(h->h_out + h->n + 2); }   // (behind the correction and the status words)
// Polls *word (acquire) until it holds seq: true when it was seen.  False after ~1 s, or as soon as a kernel has left a status
// word (a launch that gave up writes no marker): the caller then waits for the stream.
static bool wait_marker(xk_handle *h, const unsigned long long *word, unsigned long long seq) {
  bool seen = false;
  for (long spins = 0; spins < 40000000L && !(seen = (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq)); ++spins) {
    if ((spins & 255) == 255 && __atomic_load_n(&h->d_status[1], __ATOMIC_RELAXED) != 0) break;
    __builtin_ia32_pause();
  }
  return seen;
}

// Staged window lists that no kernel has carried to the device yet: one host-to-device copy through the pinned ring.
static int flush_window(xk_handle *h) {
  if (!h->win_pending) return XK_OK;
  const size_t bytes = sizeof(double) * 7 * (size_t)h->n_poses;
  double *st = (double *)stage_slot(h, bytes);
  if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
  memcpy(st, h->h_win, bytes);
  HIPCHK(h, hipMemcpyAsync(h->d_q, st, bytes, hipMemcpyHostToDevice, h->stream));
  h->win_pending = false;
  return XK_OK;
}

extern "C" int xk_stage_window(xk_handle *h, const double *C_q_G, const double *G_p_C, int n_poses) {
  if (!h || !C_q_G || !G_p_C) return XK_EINVAL;
  if (n_poses < 2 || n_poses > h->N) return fail(h, XK_ECAPACITY, "n_poses outside [2, n_poses_max]");
  HIPCHK(h, hipSetDevice(h->device));
  // Kept on the host until the next consumer.  In a filter frame that is the congruence launch of manage(), whose operand copy
  // carries the lists along (congruence()): a copy of their own runs as a ~5 us copy kernel on the frame's critical path.
  // Everything else gets them by flush_window.  Staging the same lists again (manage() and constructUpdate both do) is free.
  const bool same = h->win_valid && n_poses == h->n_poses && memcmp(h->h_win, C_q_G, sizeof(double) * 4 * n_poses) == 0 &&
                    memcmp(h->h_win + 4 * n_poses, G_p_C, sizeof(double) * 3 * n_poses) == 0;
  if (!same) {
    memcpy(h->h_win, C_q_G, sizeof(double) * 4 * n_poses);
    memcpy(h->h_win + 4 * n_poses, G_p_C, sizeof(double) * 3 * n_poses);
    h->d_p = h->d_q + 4 * (size_t)n_poses;                             // positions right behind the attitudes in use
    h->win_pending = true;
    h->win_valid = true;
    h->n_poses = n_poses;
  }
  pending_drop(h);
  h->ms_built = false;
  return XK_OK;
}

// Track staging in two halves, so that a host that builds its CSR lists anyway can build them IN the pinned staging
// memory (one pass over the tracker's lists instead of list -> vector -> staging copy; 0.2 MB at the headline size):
//   xk_stage_tracks_begin(K, n_obs, &off, &obs)  ->  fill off[0..K], obs[0..2 n_obs)  ->  xk_stage_tracks_end()
extern "C" int xk_stage_tracks_begin(xk_handle *h, int K, int n_obs, int **trk_off, double **obs_xy) {
  if (!h || K < 0 || n_obs < 0 || !trk_off || !obs_xy) return XK_EINVAL;
  if (K > h->Kmax) return fail(h, XK_ECAPACITY, "K > k_max");
  if ((size_t)n_obs > h->obs_cap) return fail(h, XK_ECAPACITY, "too many observations");
  const size_t ob = sizeof(double) * 2 * (size_t)n_obs;
  char *st = stage_slot(h, ob + sizeof(int) * (K + 1));
  if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
  h->trk_slot = st; h->trk_slot_K = K; h->trk_slot_nobs = n_obs;
  *obs_xy = (double *)st;
  *trk_off = (int *)(st + ob);
  return XK_OK;
}

extern "C" int xk_stage_tracks_end(xk_handle *h) {
  if (!h || !h->trk_slot) return XK_EINVAL;
  const int K = h->trk_slot_K;
  const size_t ob = sizeof(double) * 2 * (size_t)h->trk_slot_nobs;
  const int *trk_off = (const int *)(h->trk_slot + ob);
  char *st = h->trk_slot;
  h->trk_slot = nullptr;
  int lmax = 0;
  if (K > 0) {
    if (trk_off[0] != 0) return fail(h, XK_EINVAL, "trk_off[0] != 0");
    for (int k = 0; k < K; ++k) {
      const int L = trk_off[k + 1] - trk_off[k];
      if (L < 2 || L > h->N) return fail(h, XK_EINVAL, "track length outside [2, n_poses_max]");
      lmax = std::max(lmax, L);
    }
    if (trk_off[K] != h->trk_slot_nobs) return fail(h, XK_EINVAL, "trk_off[K] != n_obs");
    HIPCHK(h, hipSetDevice(h->device));
    h->d_trk_off = (int *)(h->d_obs + 2 * (size_t)trk_off[K]);         // offsets right behind the observations in use
    HIPCHK(h, hipMemcpyAsync(h->d_obs, st, ob + sizeof(int) * (K + 1), hipMemcpyHostToDevice, h->stream));
    memcpy(h->h_trk_off, trk_off, sizeof(int) * (K + 1));
  }
  h->K = K;
  pending_drop(h);
  h->h_pin_i[0] = lmax;                                                 // the longest track, validated against n_poses at build time
  return XK_OK;
}

extern "C" int xk_stage_tracks(xk_handle *h, const int *trk_off, const double *obs_xy, int K) {
  if (!h || K < 0 || (K > 0 && (!trk_off || !obs_xy))) return XK_EINVAL;
  if (K > 0 && trk_off[0] != 0) return fail(h, XK_EINVAL, "trk_off[0] != 0");
  if (K > 0 && trk_off[K] < 0) return fail(h, XK_EINVAL, "negative observation count");
  int *so = nullptr;
  double *sx = nullptr;
  const int rc = xk_stage_tracks_begin(h, K, K > 0 ? trk_off[K] : 0, &so, &sx);
  if (rc != XK_OK) return rc;
  if (K > 0) {
    memcpy(sx, obs_xy, sizeof(double) * 2 * (size_t)trk_off[K]);
    memcpy(so, trk_off, sizeof(int) * (K + 1));
  } else {
    so[0] = 0;
  }
  return xk_stage_tracks_end(h);
}

extern "C" int xk_chi2_quantile(double p, int dof, double *out) {
  if (!out || !(p > 0.0 && p < 1.0) || dof < 1) return XK_EINVAL;
  *out = xk_chi2_quantile_host(p, dof);
  return XK_OK;
}

// The gate of a persistent feature (slam_update.cpp:196-199): the 0.9 quantile at dof = 2 * track size, for EVERY track size -- a
// feature's track grows for as long as the feature lives.  From the table where it reaches, computed on the host past it; the handle
// remembers the last few computed ones (the features of one frame share a handful of sizes, and next frame's are one larger).
static double slam_gate_threshold(xk_handle *h, int track_size) {
  const int dof = 2 * track_size;
  if (dof < XK_CHI2_LEN) return XK_CHI2_090[dof];
  for (int i = 0; i < 8; ++i)
    if (h->chi_far_dof[i] == dof) return h->chi_far_val[i];
  const double v = xk_chi2_quantile_host(0.9, dof);
  h->chi_far_dof[h->chi_far_next] = dof;
  h->chi_far_val[h->chi_far_next] = v;
  h->chi_far_next = (h->chi_far_next + 1) % 8;
  return v;
}

extern "C" int xk_stage_slam(xk_handle *h, const double *feat, const int *anchor_idxs, const int *track_sizes,
                             const double *z_last, int M) {
  if (!h || M < 0 || (M > 0 && (!feat || !anchor_idxs || !track_sizes || !z_last))) return XK_EINVAL;
  if (M > h->Mmax) return fail(h, XK_ECAPACITY, "M > n_feat_max");
  h->anchor_max = -1;
  for (int j = 0; j < M; ++j) {   // a stale anchor (-1 in StateManager's unused slots) would index the window out of bounds, a size < 1 has no quantile
    if (anchor_idxs[j] < 0 || anchor_idxs[j] >= h->N) return fail(h, XK_EINVAL, "SLAM anchor index outside [0, n_poses_max)");
    if (track_sizes[j] < 1 || track_sizes[j] > INT_MAX / 2) return fail(h, XK_EINVAL, "SLAM track size outside [1, INT_MAX / 2]");
    h->anchor_max = std::max(h->anchor_max, anchor_idxs[j]);
  }
  if (M > 0) {
    HIPCHK(h, hipSetDevice(h->device));
    char *st = stage_slot(h, sizeof(double) * 6 * M + sizeof(int) * M);
    if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
    double *sd = (double *)st;
    int *si = (int *)(sd + 6 * M);
    memcpy(sd, feat, sizeof(double) * 3 * M);
    memcpy(sd + 3 * M, z_last, sizeof(double) * 2 * M);
    for (int j = 0; j < M; ++j) sd[5 * M + j] = slam_gate_threshold(h, track_sizes[j]);
    memcpy(si, anchor_idxs, sizeof(int) * M);
    HIPCHK(h, hipMemcpyAsync(h->d_feat, sd, sizeof(double) * 3 * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_zlast, sd + 3 * M, sizeof(double) * 2 * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_anchor, si, sizeof(int) * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_chi_s, sd + 5 * M, sizeof(double) * M, hipMemcpyHostToDevice, h->stream));
  }
  h->M = M;
  pending_drop(h);
  return XK_OK;
}

// MSCKF-SLAM tracks: the tracks whose feature becomes a persistent (SLAM) feature this frame
// (VioUpdater::constructUpdate, vio_updater.cpp:311-321).
extern "C" int xk_stage_msckf_slam(xk_handle *h, const int *trk_off, const double *obs_xy, int K2) {
  if (!h || K2 < 0 || (K2 > 0 && (!trk_off || !obs_xy))) return XK_EINVAL;
  if (K2 > h->Mmax) return fail(h, XK_ECAPACITY, "more MSCKF-SLAM tracks than feature slots");
  int lmax = 0;
  if (K2 > 0) {
    if (trk_off[0] != 0) return fail(h, XK_EINVAL, "trk_off[0] != 0");
    for (int k = 0; k < K2; ++k) {
      const int L = trk_off[k + 1] - trk_off[k];
      if (L < 2 || L > h->N) return fail(h, XK_EINVAL, "track length outside [2, n_poses_max]");
      lmax = std::max(lmax, L);
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d_trk2_off, trk_off, sizeof(int) * (K2 + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_obs2, obs_xy, sizeof(double) * 2 * trk_off[K2], hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(h->h_trk2_off, trk_off, sizeof(int) * (K2 + 1));
  }
  h->K2 = K2;
  h->ms_built = false;
  h->h_pin_i[1] = lmax;
  pending_drop(h);
  return XK_OK;
}

// LRF facet row (RangeUpdate::processRangedFacet, range_update.cpp:61-270, stacked at vio_updater.cpp:358-382).  The facet search
// (TrackManager::featureTriangleAtPoint) and the camera model stay with the caller, which passes the three SLAM feature ids and the
// undistorted, normalised image point of the LRF ray.
extern "C" int xk_stage_range(xk_handle *h, double range, double img_x_n, double img_y_n, const int facet[3], double sigma_range) {
  if (!h || !facet) return XK_EINVAL;
  if (h->M <= 0) return fail(h, XK_EINVAL, "range row without SLAM features");
  if (!(sigma_range > 0.0)) return fail(h, XK_EINVAL, "sigma_range <= 0");
  for (int j = 0; j < 3; ++j) {
    if (facet[j] < 0 || facet[j] >= h->M) return fail(h, XK_EINVAL, "facet feature id outside [0, M)");
    for (int i = 0; i < j; ++i)
      if (facet[i] == facet[j]) return fail(h, XK_EINVAL, "facet feature id repeated");
  }
  if (!std::isfinite(range) || !std::isfinite(img_x_n) || !std::isfinite(img_y_n)) return fail(h, XK_EINVAL, "non-finite range measurement");
  XkAuxIn &a = h->aux_in;
  a.range = range; a.img_x = img_x_n; a.img_y = img_y_n; a.var_range = sigma_range * sigma_range;
  for (int j = 0; j < 3; ++j) a.facet[j] = facet[j];
  h->aux_staged |= 1;
  return XK_OK;
}

// Sun-sensor rows (SolarUpdate::processSunAngle, solar_update.cpp:36-94, stacked at vio_updater.cpp:386-405).  calib (optional):
// S_q_I (w, x, y, z), G_sun (3), var_sun (deg^2) -- 8 doubles; NULL = the reference's constants (solar_update.cpp:47-56, "TODO import
// from param file": a real sensor needs its own).
extern "C" int xk_stage_sun_angle(xk_handle *h, const double q_xyzw[4], double x_angle_deg, double y_angle_deg, const double *calib) {
  if (!h || !q_xyzw) return XK_EINVAL;
  static const double ref_calib[8] = {0.360346005598587, -0.063338979194957, 0.007502445522018, 0.930635612981541,
                                      -0.29385515271891938, -0.55080445540063927, 0.78119370269565391, 10000 * 0.01777777777};
  const double *c = calib ? calib : ref_calib;
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(c[i])) return fail(h, XK_EINVAL, "non-finite sun sensor calibration");
  if (!(c[7] > 0.0)) return fail(h, XK_EINVAL, "var_sun <= 0");
  if (!(c[4] * c[4] + c[5] * c[5] + c[6] * c[6] > 0.0) || !(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3] > 0.0) ||
      !(q_xyzw[0] * q_xyzw[0] + q_xyzw[1] * q_xyzw[1] + q_xyzw[2] * q_xyzw[2] + q_xyzw[3] * q_xyzw[3] > 0.0))
    return fail(h, XK_EINVAL, "zero quaternion or sun vector");
  XkAuxIn &a = h->aux_in;
  for (int i = 0; i < 4; ++i) a.q_imu[i] = q_xyzw[i];
  a.ang[0] = x_angle_deg; a.ang[1] = y_angle_deg;
  a.s_q_i[0] = c[1]; a.s_q_i[1] = c[2]; a.s_q_i[2] = c[3]; a.s_q_i[3] = c[0];    // (w, x, y, z) -> xyzw
  for (int i = 0; i < 3; ++i) a.g_sun[i] = c[4 + i];
  a.var_sun = c[7];
  h->aux_staged |= 2;
  return XK_OK;
}

// ---------------------------------------------------------------------------
// StateManager::manage on the resident covariance
// ---------------------------------------------------------------------------
static int congruence(xk_handle *h, const int *row_ptr, const int *col_idx, const double *val, int nnz, const double *q,
                      int qdim, int qoff) {
  const int n = h->n;
  HIPCHK(h, hipSetDevice(h->device));
  // the operand goes through the pinned ring: nothing here waits for the device (a frame applies two or three of these
  // back to back -- IMU steps, manage() -- before the update's one synchronisation)
  // (+ the window lists staged since the last launch that needed them: they ride in this copy and the kernel leaves them in d_q)
  const int wn = h->win_pending ? 7 * h->n_poses : 0;
  const size_t vb = sizeof(double) * ((size_t)nnz + (q ? (size_t)qdim * qdim : 0) + wn), ib = sizeof(int) * ((size_t)n + 1 + nnz);
  char *st = stage_slot(h, vb + ib);
  if (!st) return fail(h, XK_ECAPACITY, "sparse operand exceeds the staging slot");
  double *sv = (double *)st;
  int *si = (int *)(st + vb);
  if (nnz) memcpy(sv, val, sizeof(double) * nnz);
  if (q) memcpy(sv + nnz, q, sizeof(double) * (size_t)qdim * qdim);
  const size_t woff = (size_t)nnz + (q ? (size_t)qdim * qdim : 0);
  if (wn) memcpy(sv + woff, h->h_win, sizeof(double) * wn);
  memcpy(si, row_ptr, sizeof(int) * (n + 1));
  if (nnz) memcpy(si + n + 1, col_idx, sizeof(int) * nnz);
  // [values | additive block | row pointers | column indices] in one copy
  HIPCHK(h, hipMemcpyAsync(h->d_csr_v, st, vb + ib, hipMemcpyHostToDevice, h->stream));
  double *dq = q ? h->d_csr_v + nnz : nullptr;
  const int *d_rp = (const int *)((const char *)h->d_csr_v + vb);
  XkCongArgs a{h->d_P, h->d_Pout, n, d_rp, d_rp + n + 1, h->d_csr_v, dq, qdim, qoff, wn ? h->d_csr_v + woff : nullptr, h->d_q, wn};
  h->win_pending = false;
  hipLaunchKernelGGL(xk_congruence, dim3(((size_t)n * n + 255) / 256), dim3(256), 0, h->stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, XK_EDEVICE, "congruence launch", e);
  std::swap(h->d_P, h->d_Pout);
  pending_drop(h);
  return XK_OK;
}

extern "C" int xk_cov_congruence(xk_handle *h, const int *row_ptr, const int *col_idx, const double *val, int nnz) {
  if (!h || !row_ptr || nnz < 0 || (nnz > 0 && (!col_idx || !val))) return XK_EINVAL;
  const int n = h->n;
  if (row_ptr[0] != 0 || row_ptr[n] != nnz) return fail(h, XK_EINVAL, "CSR row pointers inconsistent with nnz");
  if ((size_t)nnz > h->csr_cap) return fail(h, XK_ECAPACITY, "sparse operand has more than 24 n non-zeros");
  for (int i = 0; i < n; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) return fail(h, XK_EINVAL, "CSR row pointers not monotone");
  for (int k = 0; k < nnz; ++k)
    if (col_idx[k] < 0 || col_idx[k] >= n) return fail(h, XK_EINVAL, "CSR column index outside the state");
  return congruence(h, row_ptr, col_idx, val, nnz, nullptr, 0, 0);
}

// Propagator::propagateCovarianceMatrices (propagator.cpp:166-205) on the resident covariance:
//   P_ii <- F P_ii F^T + Q,  P_iv <- F P_iv,  P_vi <- P_vi F^T (computed on its own, as the reference insists),  P_vv kept
extern "C" int xk_cov_propagate(xk_handle *h, const double *f_d, int ldf, const double *q_d, int ldq) {
  if (!h || !f_d || !q_d || ldf < XK_CORE || ldq < XK_CORE) return XK_EINVAL;
  const int n = h->n;
  HIPCHK(h, hipSetDevice(h->device));
  XkPropArgs a;
  a.P = h->d_P; a.n = n;
  for (int c = 0; c < XK_CORE; ++c)
    for (int r = 0; r < XK_CORE; ++r) {
      a.FQ[r + XK_CORE * c] = f_d[r + (size_t)c * ldf];
      a.FQ[225 + r + XK_CORE * c] = q_d[r + (size_t)c * ldq];
    }
  hipLaunchKernelGGL(xk_cov_propagate_k, dim3(1 + (2 * (n - XK_CORE) + 255) / 256), dim3(256), 0, h->stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, XK_EDEVICE, "propagate launch", e);
  pending_drop(h);
  return XK_OK;
}

extern "C" int xk_upload_P(xk_handle *h, const double *P, int ldp, int n) {
  if (!h || !P || n != h->n || ldp < n) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy2DAsync(h->d_P, sizeof(double) * n, P, sizeof(double) * ldp, sizeof(double) * n, n,
                             hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

extern "C" int xk_download_P(xk_handle *h, double *P, int ldp, int n) {
  if (!h || !P || n != h->n || ldp < n) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy2DAsync(P, sizeof(double) * ldp, h->d_P, sizeof(double) * n, sizeof(double) * n, n,
                             hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

// Keeps / brings back a copy of the resident covariance on the device (restore = 0: save, 1: restore).  Benchmarks
// use it to replay a frame from the same prior without a PCIe upload.
extern "C" int xk_snapshot_P(xk_handle *h, int restore) {
  if (!h || restore < 0 || restore > 3) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = sizeof(double) * (size_t)h->n * h->n;
  double *&slot = (restore >= 2) ? h->d_Psnap2 : h->d_Psnap;     // 0 / 1: the caller's slot; 2 / 3: the filter loop's own (x::Ekf)
  const bool back = restore & 1;
  if (!slot) {
    if (back) return fail(h, XK_EINVAL, "xk_snapshot_P: nothing saved");
    HIPCHK(h, dalloc(&slot, (size_t)h->n * h->n));
  }
  HIPCHK(h, hipMemcpyAsync(back ? h->d_P : slot, back ? slot : h->d_P, bytes, hipMemcpyDeviceToDevice, h->stream));
  return XK_OK;
}

extern "C" int xk_msckf_slam_results(xk_handle *h, int *inlier, double *gamma, double *H1, int ldh1, double *H2, int ldh2,
                                     double *r1, double *features) {
  if (!h) return XK_EINVAL;
  const int k = h->K2, n = h->n;
  if (k == 0) return XK_OK;
  if (!h->ms_built) return fail(h, XK_EINVAL, "xk_msckf_build has not run on the staged MSCKF-SLAM tracks");
  if ((H1 && ldh1 < 3 * k) || (H2 && ldh2 < 3 * k)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> h1((size_t)3 * k * n), h2((size_t)9 * k);
  if (inlier) HIPCHK(h, hipMemcpyAsync(inlier, h->d_inl2, sizeof(int) * k, hipMemcpyDeviceToHost, h->stream));
  if (gamma) HIPCHK(h, hipMemcpyAsync(gamma, h->d_gam2, sizeof(double) * k, hipMemcpyDeviceToHost, h->stream));
  if (r1) HIPCHK(h, hipMemcpyAsync(r1, h->d_r1, sizeof(double) * 3 * k, hipMemcpyDeviceToHost, h->stream));
  if (features) HIPCHK(h, hipMemcpyAsync(features, h->d_feat2, sizeof(double) * 3 * k, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h1.data(), h->d_H1, sizeof(double) * h1.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h2.data(), h->d_H2, sizeof(double) * h2.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (H1)     // device: [track][3][n] row-major -> (3k x n) column-major
    for (int j = 0; j < k; ++j)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < n; ++c) H1[(size_t)(3 * j + r) + (size_t)c * ldh1] = h1[((size_t)j * 3 + r) * n + c];
  if (H2) {   // block diagonal (msckf_slam_update.cpp:231)
    for (int c = 0; c < 3 * k; ++c)
      for (int r = 0; r < 3 * k; ++r) H2[r + (size_t)c * ldh2] = 0.0;
    for (int j = 0; j < k; ++j)
      for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) H2[(size_t)(3 * j + r) + (size_t)(3 * j + c) * ldh2] = h2[9 * (size_t)j + r + 3 * c];
  }
  return XK_OK;
}

static bool inv3(const double *a /*col-major*/, double *o) {
  const double c00 = a[4] * a[8] - a[7] * a[5], c01 = a[7] * a[2] - a[1] * a[8], c02 = a[1] * a[5] - a[4] * a[2];
  const double det = a[0] * c00 + a[3] * c01 + a[6] * c02;
  if (!(fabs(det) > 0.0)) return false;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
  o[3] = (a[6] * a[5] - a[3] * a[8]) * id; o[4] = (a[0] * a[8] - a[6] * a[2]) * id; o[5] = (a[3] * a[2] - a[0] * a[5]) * id;
  o[6] = (a[3] * a[7] - a[6] * a[4]) * id; o[7] = (a[6] * a[1] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[3] * a[1]) * id;
  return true;
}

// StateManager::initMsckfSlamFeatures + addFeatureStates (state_manager.cpp:151-174,199-226) on the resident
// covariance: with G = H2^-1 H1 the new feature states are  f - G corr + H2^-1 r1,  their covariance blocks
// -G P (cross) and G P G^T + sigma^2 H2^-1 H2^-T (diagonal) -- one congruence with J = [I; -G] on the rows of
// the new features plus the noise block.
extern "C" int xk_init_msckf_slam_features(xk_handle *h, int n_features, const double *correction, double sigma_img,
                                           double *new_features) {
  if (!h || !correction || !new_features || n_features < 0 || !(sigma_img > 0.0)) return XK_EINVAL;
  const int k = h->K2, n = h->n;
  if (k == 0) return XK_OK;
  if (!h->ms_built) return fail(h, XK_EINVAL, "xk_msckf_build has not run on the staged MSCKF-SLAM tracks");
  if (n_features + k > h->Mmax) return fail(h, XK_ECAPACITY, "not enough free feature slots");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> h1((size_t)3 * k * n), h2((size_t)9 * k), r1((size_t)3 * k), f((size_t)3 * k);
  HIPCHK(h, hipMemcpyAsync(h1.data(), h->d_H1, sizeof(double) * h1.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h2.data(), h->d_H2, sizeof(double) * h2.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(r1.data(), h->d_r1, sizeof(double) * r1.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(f.data(), h->d_feat2, sizeof(double) * f.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int ns = XK_CORE + 6 * h->N + 3 * n_features;     // first row of the new features
  const double var_img = sigma_img * sigma_img;
  std::vector<double> G((size_t)3 * k * n, 0.0), Q((size_t)9 * k * k, 0.0);
  for (int j = 0; j < k; ++j) {
    double hi[9];
    if (!inv3(&h2[9 * (size_t)j], hi)) return fail(h, XK_ESINGULAR, "H2 is singular (camera hovering)");   // state_manager.cpp:158-160
    for (int r = 0; r < 3; ++r) {
      double *g = &G[((size_t)3 * j + r) * n];
      for (int c = 0; c < n; ++c)
        g[c] = hi[r] * h1[((size_t)j * 3) * n + c] + hi[r + 3] * h1[((size_t)j * 3 + 1) * n + c] + hi[r + 6] * h1[((size_t)j * 3 + 2) * n + c];
      double fr = f[3 * j + r] + hi[r] * r1[3 * j] + hi[r + 3] * r1[3 * j + 1] + hi[r + 6] * r1[3 * j + 2];
      for (int c = 0; c < n; ++c) fr -= g[c] * correction[c];
      new_features[3 * j + r] = fr;
      for (int c2 = 0; c2 < 3; ++c2)      // sigma^2 H2^-1 H2^-T, block (j, j)
        Q[(size_t)(3 * j + r) + (size_t)(3 * j + c2) * 3 * k] = var_img * (hi[r] * hi[c2] + hi[r + 3] * hi[c2 + 3] + hi[r + 6] * hi[c2 + 6]);
    }
  }
  std::vector<int> rp(n + 1), ci;
  std::vector<double> v;
  for (int r = 0; r < n; ++r) {
    rp[r] = (int)ci.size();
    if (r >= ns && r < ns + 3 * k) {
      const double *g = &G[(size_t)(r - ns) * n];
      for (int c = 0; c < n; ++c)
        if (g[c] != 0.0) { ci.push_back(c); v.push_back(-g[c]); }
    } else {
      ci.push_back(r);
      v.push_back(1.0);
    }
  }
  rp[n] = (int)ci.size();
  if (ci.size() > h->csr_cap) return fail(h, XK_ECAPACITY, "sparse operand too large");
  return congruence(h, rp.data(), ci.data(), v.data(), (int)ci.size(), Q.data(), 3 * k, ns);
}

// StateManager::initStandardSlamFeatures + addFeatureStates (state_manager.cpp:176-226): k new features with no
// correlation to the rest, variances sigma_img^2, sigma_img^2, sigma_rho_0^2.
extern "C" int xk_init_standard_slam_features(xk_handle *h, int n_features, int k, double sigma_img, double sigma_rho_0) {
  if (!h || n_features < 0 || k < 0) return XK_EINVAL;
  if (k == 0) return XK_OK;
  if (n_features + k > h->Mmax) return fail(h, XK_ECAPACITY, "not enough free feature slots");
  const int n = h->n, ns = XK_CORE + 6 * h->N + 3 * n_features;
  std::vector<int> rp(n + 1), ci;
  std::vector<double> v, Q((size_t)9 * k * k, 0.0);
  for (int r = 0; r < n; ++r) {
    rp[r] = (int)ci.size();
    if (r < ns || r >= ns + 3 * k) { ci.push_back(r); v.push_back(1.0); }
  }
  rp[n] = (int)ci.size();
  for (int j = 0; j < 3 * k; ++j) Q[(size_t)j + (size_t)j * 3 * k] = (j % 3 == 2) ? sigma_rho_0 * sigma_rho_0 : sigma_img * sigma_img;
  return congruence(h, rp.data(), ci.data(), v.data(), (int)ci.size(), Q.data(), 3 * k, ns);
}

// ---------------------------------------------------------------------------
// the update path: rows, compression, Kalman update, the staged and queued entries, xk_apply_update, measurement
// ---------------------------------------------------------------------------
#include "xk_update_api.hip.h"

// ---------------------------------------------------------------------------
// covariance intersection: the fuse / match / track entries, applyCI, the device-resident round, the inter-agent payload
// ---------------------------------------------------------------------------
#include "xk_ci_api.hip.h"

// ---------------------------------------------------------------------------
// fp64 ceiling probe (lab build only: include/xk_lab.h)
// ---------------------------------------------------------------------------
#ifdef XK_LAB
__global__ __launch_bounds__(256) void xk_probe_mfma(double *out, int iters) {
  xk_d4 a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0;
  const double x = 1.0 + threadIdx.x * 1e-9, y = 1.0 - threadIdx.x * 1e-9;
  for (int i = 0; i < iters; ++i) {
    a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y, x, a1, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, a2, 0, 0, 0);
    a3 = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, a3, 0, 0, 0);
  }
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = a0[0] + a1[1] + a2[2] + a3[3];
}
__global__ __launch_bounds__(256) void xk_probe_fma(double *out, int iters) {
  double a[8];
  const double x = 1.0 + threadIdx.x * 1e-9, y = 1e-9 * threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = k;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = fma(a[k], x, y);
  }
  double s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += a[k];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

extern "C" int xk_probe_fp64_peak(xk_handle *h, int use_mfma, double *tflops) {
  if (!h || !tflops) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const int blocks = 256 * 8, iters = 20000;
  double *buf = nullptr;
  HIPCHK(h, hipMalloc((void **)&buf, sizeof(double) * blocks * 256));
  for (int rep = 0; rep < 2; ++rep) {
    HIPCHK(h, hipEventRecord(h->ev[8], h->stream));
    if (use_mfma) hipLaunchKernelGGL(xk_probe_mfma, dim3(blocks), dim3(256), 0, h->stream, buf, iters);
    else hipLaunchKernelGGL(xk_probe_fma, dim3(blocks), dim3(256), 0, h->stream, buf, iters);
    HIPCHK(h, hipEventRecord(h->ev[9], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  float ms = 0;
  hipEventElapsedTime(&ms, h->ev[8], h->ev[9]);
  hipFree(buf);
  const double waves = (double)blocks * 4;
  const double flops = use_mfma ? waves * iters * 4.0 * (2.0 * 16 * 16 * 4) : waves * 64.0 * iters * 8.0 * 2.0;
  *tflops = flops / (ms * 1e-3) / 1e12;
  return XK_OK;
}
#endif   // XK_LAB

extern "C" int xk_set_option(xk_handle *h, const char *name, int value) {
  if (!h || !name) return XK_EINVAL;
  // operational switches of the release library: the schedule of the compression and how soon a fast path that gave up is retried
  if (!strcmp(name, "caqr_resident")) h->opt_resident = value;
  else if (!strcmp(name, "caqr_rearm")) h->rearm_after = value;
  else if (!strcmp(name, "caqr_tail")) h->opt_tail = value;
  else if (!strcmp(name, "slam_split")) h->opt_slam_split = value;
  else if (!strcmp(name, "ci_weight_search")) {
    if (value != 0 && value != 1) return fail(h, XK_EINVAL, "xk_set_option: ci_weight_search is 0 or 1");
    h->opt_ci_search = value;
  }
#ifdef XK_LAB
  // test hooks and A/B switches (include/xk_lab.h)
  else if (!strcmp(name, "caqr_poison")) h->opt_poison = value;
  else if (!strcmp(name, "caqr_test_stall")) h->opt_test_stall = value;
  else if (!strcmp(name, "caqr_tall26")) h->opt_tall26 = value;
  else if (!strcmp(name, "pipe_kalman")) h->opt_kalman = value;
  else if (!strcmp(name, "pipe_split")) { if (h->opt_split >= 0) h->opt_split = value; }
  else if (!strcmp(name, "caqr_hlite")) h->opt_hlite = value;
  else if (!strcmp(name, "feat_gate_form")) h->opt_gate_form = value ? 1 : 0;   // A/B switch, and the tests' handle on the fallback
  else if (!strcmp(name, "photo_spatial_cap")) h->opt_psp_cap = value > 0 ? value : 0;   // the tests' handle on a solve that does not converge
#endif
  else return fail(h, XK_EINVAL, "xk_set_option: unknown option");
  return XK_OK;
}

// Which schedule compressed the last update, and how the fast path has fared on this handle (include/xk.h).
extern "C" int xk_caqr_status(const xk_handle *h, int *schedule, int *armed, int *giveups, int *last_reason) {
  if (!h) return XK_EINVAL;
  if (schedule) *schedule = outcome_status(h->last);
  if (armed) *armed = (h->persist_ok || h->tail_ok) ? 1 : 0;
  if (giveups) *giveups = h->fast_giveups;
  if (last_reason) *last_reason = h->fast_reason;
  return XK_OK;
}

#ifdef XK_LAB
extern "C" int xk_is_lab(void) { return 1; }
// Wall-clock (100 MHz) stamps of the last single-launch CAQR (XK_CAQR_PERSIST_DBG=1): per panel k, out[8k + 0..5] = role-T
// workgroup (XCD 0, slot 0): tile step start / end, after barrier 1, first-level merge start, end, after barrier 2;
// out[8k + 6..7] = last-level workgroup 0: roots complete -> its strips published.  tools/exp/persist_trace.py prints them.
extern "C" int xk_debug_persist_stamps(xk_handle *h, long long *out, int n_out) {
  if (!h || !out || !h->d_pdbg) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_pdbg, sizeof(long long) * (size_t)std::min(n_out, XK_PDBG_WORDS), hipMemcpyDeviceToHost));
  return XK_OK;
}
// The triangulated landmarks and Gauss-Newton iteration counts of the last build's tracks (include/xk_lab.h): d_gpf / d_gn as xk_msckf_feature left them.
extern "C" int xk_debug_feature_points(xk_handle *h, double *gpf, int *gn_iters, int K) {
  if (!h || !gpf || !gn_iters || K < 0 || K != h->K) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (K == 0) return XK_OK;
  HIPCHK(h, hipMemcpy(gpf, h->d_gpf, sizeof(double) * 3 * (size_t)K, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(gn_iters, h->d_gn, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost));
  return XK_OK;
}

extern "C" int xk_debug_stack_rows(xk_handle *h, int slot, int nrows, double *out) {
  if (!h || !out || slot < 0 || nrows < 0 || (long)slot * h->DB + nrows > (long)h->ntiles_max * h->DB) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nrows == 0) return XK_OK;
  HIPCHK(h, hipMemcpy2D(out, sizeof(double) * (h->na + 1), h->d_A + (size_t)slot * h->DB * h->C1P, sizeof(double) * h->C1P,
                        sizeof(double) * (h->na + 1), (size_t)nrows, hipMemcpyDeviceToHost));
  return XK_OK;
}
#endif   // XK_LAB

#if defined(XK_FEAT_PROBE) && defined(XK_LAB)
extern "C" int xk_debug_feature_phases(xk_handle *h, double sigma_img, long long *out, int n_out) {
  // out[12k ..]: 8 clock64 phase stamps, wall start, wall end, (XCC_ID << 32 | HW_ID) of workgroup k
  const size_t bytes = sizeof(long long) * (size_t)(12 * h->K);
  hipMalloc((void **)&h->feat_dbg, bytes);
  hipMemset(h->feat_dbg, 0, bytes);
  int rc = launch_build(h, sigma_img);
  hipStreamSynchronize(h->stream);
  hipMemcpy(out, h->feat_dbg, std::min(bytes, sizeof(long long) * (size_t)n_out), hipMemcpyDeviceToHost);
  hipFree(h->feat_dbg);
  h->feat_dbg = nullptr;
  return rc;
}
#endif

// ---------------------------------------------------------------------------
// The vision stages in front of the filter: place recognition (xk_pr_*) and the tracker's front end (xk_trk_*).  Their host
// side lives in the two headers included below; their RANSAC filters share xk_ransac.hip.h.
// ---------------------------------------------------------------------------
#include "xk_ransac.hip.h"

// What the last RANSAC of a filter left for hypotheses first ... first+count-1, behind `who`: the three optional copies and one
// wait.  n_hyp: hypotheses of that RANSAC (`last` names it in the error text), -1 before the scratch block exists.
static int ransac_hypotheses(xk_handle *h, const char *who, const char *last, int n_hyp, const XkRansacScratch &s, int maxc, int first,
                             int count, int *n_cand, double *cand, int *inliers) {
  char msg[160];
  if (first < 0 || count < 0) {
    snprintf(msg, sizeof msg, "%s: negative range", who);
    return fail(h, XK_EINVAL, msg);
  }
  if (first + (long)count > n_hyp) {
    snprintf(msg, sizeof msg, "%s: range outside the hypotheses of the last %s", who, last);
    return fail(h, XK_EINVAL, msg);
  }
  if (count == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t per = (size_t)maxc;
  if (n_cand) HIPCHK(h, hipMemcpyAsync(n_cand, s.ncand + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
  if (cand)
    HIPCHK(h, hipMemcpyAsync(cand, s.cand + first * per * 9, sizeof(double) * count * per * 9, hipMemcpyDeviceToHost, h->stream));
  if (inliers)
    HIPCHK(h, hipMemcpyAsync(inliers, s.cnt + first * per, sizeof(int) * count * per, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

#include "xk_place_api.hip.h"
#include "xk_tracker_api.hip.h"
