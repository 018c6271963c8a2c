// xk_api.hip -- C ABI (include/xk.h) of the MI355X-native xVIO EKF-update engine.
// Host-side orchestration only: every number in a result is produced by the
// HIP kernels in xk_feature.hip.h / xk_linalg.hip.h / xk_ci.hip.h.
#include "../../include/xk.h"
#ifdef XK_LAB
#include "../../include/xk_lab.h"
#endif

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "xk_chi2_table.h"
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
  h->d_p = h->d_q + 4 * (size_t)n_poses_max;
  HIPCHK(h, dalloc(&h->d_obs, 2 * h->obs_cap + ((size_t)k_max + 2) / 2 + 1));
  h->d_trk_off = (int *)(h->d_obs + 2 * h->obs_cap);
  HIPCHK(h, dalloc(&h->d_feat, 3 * (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_zlast, 2 * (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_anchor, (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_tsz, (size_t)n_feat_max));
  HIPCHK(h, dalloc(&h->d_P, nn));
  HIPCHK(h, dalloc(&h->d_Pout, nn));
  HIPCHK(h, dalloc(&h->d_fq, (size_t)450));
  HIPCHK(h, dalloc(&h->d_chi95, (size_t)XK_CHI2_LEN));
  HIPCHK(h, dalloc(&h->d_chi90, (size_t)XK_CHI2_LEN));
  HIPCHK(h, hipMemcpy(h->d_chi95, XK_CHI2_095, sizeof(double) * XK_CHI2_LEN, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_chi90, XK_CHI2_090, sizeof(double) * XK_CHI2_LEN, hipMemcpyHostToDevice));
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
  void *ptrs[] = {h->d_q, h->d_obs, h->d_feat, h->d_zlast, h->d_anchor, h->d_tsz,
                  h->d_P, h->d_Pout, h->d_chi95, h->d_chi90, h->d_A, h->d_tile_rows, h->d_panel[0], h->d_panel[1], h->d_inl, h->d_inl_s,
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
  delete h->fused_ct;
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
  h->have_rows = h->have_R = false;
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
  h->have_rows = h->have_R = false;
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

extern "C" int xk_stage_slam(xk_handle *h, const double *feat, const int *anchor_idxs, const int *track_sizes,
                             const double *z_last, int M) {
  if (!h || M < 0 || (M > 0 && (!feat || !anchor_idxs || !track_sizes || !z_last))) return XK_EINVAL;
  if (M > h->Mmax) return fail(h, XK_ECAPACITY, "M > n_feat_max");
  h->anchor_max = -1;
  for (int j = 0; j < M; ++j) {   // a stale anchor (-1 in StateManager's unused slots) or size would index the window / chi-square table out of bounds
    if (anchor_idxs[j] < 0 || anchor_idxs[j] >= h->N) return fail(h, XK_EINVAL, "SLAM anchor index outside [0, n_poses_max)");
    if (track_sizes[j] < 1) return fail(h, XK_EINVAL, "SLAM track size < 1");
    h->anchor_max = std::max(h->anchor_max, anchor_idxs[j]);
  }
  if (M > 0) {
    HIPCHK(h, hipSetDevice(h->device));
    char *st = stage_slot(h, sizeof(double) * 6 * M);
    if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
    double *sd = (double *)st;
    int *si = (int *)(sd + 5 * M);
    memcpy(sd, feat, sizeof(double) * 3 * M);
    memcpy(sd + 3 * M, z_last, sizeof(double) * 2 * M);
    memcpy(si, anchor_idxs, sizeof(int) * M);
    memcpy(si + M, track_sizes, sizeof(int) * M);
    HIPCHK(h, hipMemcpyAsync(h->d_feat, sd, sizeof(double) * 3 * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_zlast, sd + 3 * M, sizeof(double) * 2 * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_anchor, si, sizeof(int) * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_tsz, si + M, sizeof(int) * M, hipMemcpyHostToDevice, h->stream));
  }
  h->M = M;
  h->have_rows = h->have_R = false;
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
  h->have_rows = h->have_R = false;
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

static int congruence(xk_handle *h, const int *row_ptr, const int *col_idx, const double *val, int nnz, const double *q,
                      int qdim, int qoff);

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
    s.feat = h->d_feat; s.anchor_idxs = h->d_anchor; s.track_sizes = h->d_tsz; s.z_last = h->d_zlast; s.M = h->M;
    s.P = h->d_P; s.n = h->n; s.var_img = sigma_img * sigma_img; s.chi90 = h->d_chi90; s.chi_len = XK_CHI2_LEN;
    s.A = h->d_A + (size_t)(h->K + h->K2) * h->DB * h->C1P; s.DB = h->DB; s.C1P = h->C1P; s.na = h->na;
    s.inlier = h->d_inl_s; s.gamma = h->d_gam_s;
    if (h->K > 0 && !h->feat_dbg && !xk_feature_packed(h->n_poses)) hipLaunchKernelGGL(xk_build_rows, dim3(h->K + h->M), dim3(XK_FEAT_THREADS), feat_lds, h->stream, fa, s);
    else hipLaunchKernelGGL(xk_slam_rows, dim3(h->M), dim3(64), 0, h->stream, s);
    // rows per SLAM tile (gated-out features leave zero rows, as in the reference)
    std::vector<int> tr(slam_tiles);
    for (int t = 0; t < slam_tiles; ++t) tr[t] = std::min(h->DB, 2 * h->M - t * h->DB);
    for (int t = 0; t < slam_tiles; ++t) h->h_pin_i[8 + t] = tr[t];
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
  h->have_rows = true;
  h->have_R = false;
  h->compress_deferred = false;
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


// Kalman algebra on the device (updater.cpp:117-141 / :144-161).  ev (optional)
// = {before, after-gemm-part...} is not used here; stage split is timed by the caller.
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
  int rc = launch_compress(h);
  if (rc == XK_OK) rc = read_status(h, true);
  if (rc == XK_RETRY_CLASSIC) {                  // rebuild the rows (the tiles were worked on in place) and compress the slow way
    if ((rc = launch_build(h, h->sigma_img, true)) == XK_OK && (rc = launch_compress(h)) == XK_OK) rc = read_status(h);
  }
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
  h->compress_deferred = h->opt_resident && h->persist_ok && kalman_rides(h) &&
                         h->K + h->K2 + h->M > 0 && h->plan < 2 &&   // (stacks that are not compressed at all: nothing to defer)
                         h->naux == 0;   // (range / sun rows: the update is not taken along by the launch anyway)
  if (h->compress_deferred) h->have_R = true;     // (as far as xk_apply_update's precondition goes: it runs the compression itself)
  else if ((rc = launch_compress(h)) != XK_OK) return rc;
  h->async_pending = true;
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
  bool ct_zero = true;
  if (corr_total)
    for (int i = 0; i < h->n && ct_zero; ++i) ct_zero = corr_total[i] == 0.0;
  const double *dct = nullptr;
  if (!ct_zero) {
    double *st = (double *)stage_slot(h, sizeof(double) * h->n);
    if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
    memcpy(st, corr_total, sizeof(double) * h->n);
    HIPCHK(h, hipMemcpyAsync(h->d_ct, st, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    dct = h->d_ct;
  }
  int rc = launch_build(h, sigma_img);
  if (rc != XK_OK) return rc;
  if ((rc = cache_flags(h)) != XK_OK) return rc;
  UpdateSpec u = compressed_spec(h, dct, cov_update ? 1 : 0);
  u.corr = h->h_out;
  const int spin_env = spin_done();
  if (spin_env) { u.done_flag = reinterpret_cast<unsigned long long *>(h->h_out + h->n + 2); u.done_seq = ++h->done_seq; }
  if ((rc = launch_compress(h, nullptr, &u)) != XK_OK) return rc;
  if (!h->last.fused && (rc = launch_update(h, u)) != XK_OK) return rc;
  h->async_pending = true;
  h->fused_pending = true;
  h->fused_seq = spin_env ? u.done_seq : 0;
  h->fused_cov_update = cov_update ? 1 : 0;
  h->fused_ct_zero = ct_zero;
  if (!h->fused_ct) h->fused_ct = new std::vector<double>();
  if (ct_zero) h->fused_ct->clear(); else h->fused_ct->assign(corr_total, corr_total + h->n);
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
  if (!h->have_R) return fail(h, XK_EINVAL, "xk_qr_compress has not run on the staged inputs");
  HIPCHK(h, hipSetDevice(h->device));
  const double *dct = nullptr;
  bool ct_zero = true;                                 // Updater::update starts every update from a zero correction_total
  if (corr_total)
    for (int i = 0; i < h->n && ct_zero; ++i) ct_zero = corr_total[i] == 0.0;
  // arguments first, before any state of the handle is touched: a mismatch with what xk_build_compress_update_async queued leaves the
  // queued update (posterior in d_Pout, marker, retry bookkeeping) exactly as it was -- the matching call can still collect it
  if (h->fused_pending) {
    bool same = (cov_update ? 1 : 0) == h->fused_cov_update && ct_zero == h->fused_ct_zero;
    if (same && !ct_zero) same = memcmp(corr_total, h->fused_ct->data(), sizeof(double) * h->n) == 0;
    if (!same) return fail(h, XK_EINVAL, "xk_apply_update: not the correction_total / cov_update the queued pass was built with");
  }
  if (corr_total && !ct_zero) {
    double *st = (double *)stage_slot(h, sizeof(double) * h->n);
    if (!st) return fail(h, XK_ECAPACITY, "staging slot too small");
    memcpy(st, corr_total, sizeof(double) * h->n);
    HIPCHK(h, hipMemcpyAsync(h->d_ct, st, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    dct = h->d_ct;
  }
  const bool deferred = h->compress_deferred;
  const bool async = h->async_pending || deferred, queued = h->fused_pending;
  h->async_pending = false;
  h->fused_pending = false;
  h->compress_deferred = false;
  int rc = XK_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (attempt == 1) {   // the single-launch CAQR of xk_build_compress_async gave up: rows, compression and update again
      if (deferred) {
        // ... NOT the rows: they were linearised and gated at the prior, which the applyCI entries have replaced since -- and they
        // are still there (the single launch only reads the tiles / factor records; it is the multi-launch schedule that works
        // on the tiles in place, and it has not run)
        h->have_rows = true;
      } else {
        if ((rc = launch_build(h, h->sigma_img, true)) != XK_OK) return rc;
        if ((rc = cache_flags(h)) != XK_OK) return rc;
      }
      if ((rc = launch_compress(h)) != XK_OK) return rc;
    }
    UpdateSpec u = compressed_spec(h, dct, cov_update);
    u.corr = h->h_out;
    const bool waiting_only = queued && attempt == 0;      // the update is already on the stream (xk_build_compress_update_async)
    // The kernels write the correction and (on failure) the status words into pinned host memory; the last workgroup of the
    // last launch then writes a sequence number next to them, which the host polls: the results are there ~5 us before the
    // runtime's completion signal says so (XK_SPIN_DONE=0: wait for that signal instead).  One wait per update, no copy.
    const int spin_env = spin_done();
    unsigned long long *done = reinterpret_cast<unsigned long long *>(h->h_out + h->n + 2);
    if (waiting_only) u.done_seq = h->fused_seq;
    else {
      if (spin_env) { u.done_flag = done; u.done_seq = ++h->done_seq; }
      if (deferred && attempt == 0) {                      // the compression xk_build_compress_async left for now, Kalman role inside
        if ((rc = launch_compress(h, nullptr, &u)) != XK_OK) return rc;
        rc = h->last.fused ? XK_OK : launch_update(h, u);
      } else rc = launch_update(h, u);
      if (rc != XK_OK) return rc;
    }
    bool seen = false;
    if (spin_env && u.done_seq) {
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
      seen = wait_marker(h, done, u.done_seq);
      if (seen) h->done_seen = u.done_seq;
    }
    if (!seen) HIPCHK(h, hipStreamSynchronize(h->stream));
    stage_stream_idle(h);
    rc = eval_status(h, h->d_status[0], h->d_status[1], async && attempt == 0);
    if (rc != XK_RETRY_CLASSIC) break;
  }
  if (rc != XK_OK) return rc;
  memcpy(correction, h->h_out, sizeof(double) * h->n);
  std::swap(h->d_P, h->d_Pout);  // posterior becomes the resident covariance
  h->have_rows = h->have_R = false;
  return XK_OK;
}

extern "C" int xk_visual_update_staged(xk_handle *h, double sigma_img, double *correction, int *inlier_msckf,
                                       double *gamma_msckf, int *inlier_slam, double *gamma_slam) {
  if (!h || !correction || !(sigma_img > 0.0)) return XK_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->K == 0 && h->K2 == 0 && h->M == 0 && !h->aux_staged) {  // h.size() == 0 -> no update (updater.cpp:106); MSCKF-SLAM rows count (vio_updater.cpp:413-419)
    for (int i = 0; i < h->n; ++i) correction[i] = 0.0;
    h->last.schedule = XK_SCHED_EMPTY;            // (xk_caqr_status: 4; staging cleared have_R, or the compression it stands for was of this same empty stack: nothing else reads the record before the next one)
    return XK_OK;
  }
  int rc = XK_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    rc = launch_build(h, sigma_img, attempt > 0);
    if (rc != XK_OK) return rc;
    UpdateSpec u = compressed_spec(h, nullptr, 1);
    rc = launch_compress(h, nullptr, &u);            // (the single launch takes the Kalman update along where it can)
    if (rc != XK_OK) return rc;
    if (!h->last.fused) rc = launch_update(h, u);
    if (rc != XK_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(correction, h->d_corr, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    rc = fetch_flags(h, inlier_msckf, gamma_msckf, inlier_slam, gamma_slam);
    if (rc != XK_OK) return rc;
    rc = read_status(h, attempt == 0);
    if (rc != XK_RETRY_CLASSIC) break;           // (the prior is untouched in d_P: the whole update is simply redone)
  }
  if (rc != XK_OK) return rc;
  std::swap(h->d_P, h->d_Pout);
  h->have_rows = h->have_R = false;
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
  if (!h->async_pending) return XK_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  stage_stream_idle(h);
  int rc = eval_status(h, h->d_status[0], h->d_status[1], true);
  if (rc == XK_RETRY_CLASSIC) {
    if ((rc = launch_build(h, h->sigma_img, true)) != XK_OK) return rc;
    if ((rc = cache_flags(h)) != XK_OK) return rc;
    if ((rc = launch_compress(h)) != XK_OK) return rc;
  }
  if (rc == XK_OK) h->async_pending = false;
  return rc;
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
  for (int attempt = 0; attempt < 2; ++attempt) {
  for (int s = 0; s < XK_NSTAGE; ++s) acc[s] = 0;
  tot = 0;
  for (int it = 0; it < warmup + steps; ++it) {
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    int rc = launch_build(h, sigma_img, attempt > 0 || it > 0);   // (staged range / sun rows: in every step)
    if (rc != XK_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    UpdateSpec u = compressed_spec(h, nullptr, 1);
    rc = launch_compress(h, h->ev[2], &u);
    if (rc != XK_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
    if (!h->last.fused) rc = launch_update(h, u);     // (fused: the Kalman update is inside stage 2's launch, stage 4 reads 0)
    if (rc != XK_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
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
  const int rc = read_status(h, attempt == 0);
  if (rc == XK_RETRY_CLASSIC) continue;            // the single-launch CAQR gave up somewhere: measure the multi-launch schedule
  if (rc != XK_OK) return rc;
  break;
  }
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

// ---------------------------------------------------------------------------
// covariance intersection: the fuse / match / track entries, applyCI, the device-resident round, the inter-agent payload
// ---------------------------------------------------------------------------
#include "xk_ci_api.hip.h"

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
  h->have_rows = h->have_R = false;
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
  h->have_rows = h->have_R = false;
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
    int rc = launch_build(h, sigma_img);
    if (rc == XK_OK) rc = launch_compress(h);
    if (rc == XK_OK) { UpdateSpec u = compressed_spec(h, nullptr, 1); rc = launch_update(h, u); }
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
  for (int attempt = 0; attempt < 2; ++attempt) {
    for (int it = 0; it < steps; ++it) {
      int rc = launch_build(h, sigma_img, attempt > 0 || it > 0);   // (staged range / sun rows: in every step)
      if (rc != XK_OK) return rc;
      UpdateSpec u = compressed_spec(h, nullptr, 1);
      rc = launch_compress(h, nullptr, &u);
      if (rc != XK_OK) return rc;
      if (!h->last.fused) rc = launch_update(h, u);
      if (rc != XK_OK) return rc;
    }
    const int rc = read_status(h, attempt == 0);
    if (rc != XK_RETRY_CLASSIC) return rc;
  }
  return XK_EDEVICE;
}

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
