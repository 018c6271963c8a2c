// xk_place_api.hip.h -- host side of the place-recognition entries (xk_pr_*): the request filter and keyframe store
// and the training of the vocabulary they consume (xk_voc_*, at the end)
// (the component either side of the CI exchange on the communication axis; mirrors VLAD / Database /
// Keyframe of src/x/place_recognition) and the essential-matrix RANSAC filter of findCorrespondences.  Part of xk_api.hip's
// translation unit, included at its end.
#pragma once
#include "xk_place.hip.h"
#include "xk_essential.hip.h"
#include "xk_correspond.hip.h"
#include "xk_vocab.hip.h"

#define XK_PR_MAX_KEYFRAMES 15   // database.h:70

struct xk_pr {
  xk_handle *h;
  int k, L, n_nodes, kmax, W, n_words, clusters, VW, max_desc;
  long pay_n, trk_n;
  unsigned int *d_node_desc;
  int *d_children, *d_word_of_node, *d_node_of_word;
  // keyframe store: slot s of the ring holds one keyframe; order[] lists the live slots oldest first
  unsigned int *d_vlad;       // [15][VW]
  unsigned int *d_kfdesc;     // [15][max_desc][W]
  double *d_payload;          // [15][pay_n]
  double *d_tracks;           // [15][trk_n]
  int n_desc[XK_PR_MAX_KEYFRAMES];
  long tag[XK_PR_MAX_KEYFRAMES];
  std::vector<int> *uav_ids[XK_PR_MAX_KEYFRAMES];   // Keyframe::uav_ids_ (a std::set in the reference)
  int order[XK_PR_MAX_KEYFRAMES], live;
  // scratch
  unsigned int *d_q, *d_t, *d_qvlad;
  int *d_ham, *d_knn;
  int *h_int;                 // pinned
  unsigned int *h_words;      // pinned staging for descriptors / VLADs
  size_t h_words_cap;
  // essential-matrix RANSAC (xk_essential.hip.h): allocated by the first xk_pr_essential_ransac, not by xk_pr_create
  unsigned char *d_ess;       // XkRansacScratch | E [9] | res [2] | pixel pairs [4 max_desc] floats | mask [max_desc]
  unsigned char *h_ess;       // pinned: pixel pairs in, E / n_inliers / winner / mask out
  int ess_n_hyp;              // hypotheses of the last call (0: none yet)
  // findCorrespondences in one call (xk_correspond.hip.h): allocated by the first xk_pr_find_correspondences
  unsigned char *d_corr;      // input block | G, first_j, alive, count | result block, each sized by max_desc
  unsigned char *h_corr;      // pinned: input block | result block of the last call
  int corr_n_rec;             // bound the last call's result block is laid out by (-1 after a failed call); corr_called: any call yet
  bool corr_called;
};

extern "C" void xk_pr_destroy(xk_pr *p) {
  if (!p) return;
  hipFree(p->d_node_desc); hipFree(p->d_children); hipFree(p->d_word_of_node); hipFree(p->d_node_of_word);
  hipFree(p->d_vlad); hipFree(p->d_kfdesc); hipFree(p->d_payload); hipFree(p->d_tracks);
  hipFree(p->d_q); hipFree(p->d_t); hipFree(p->d_qvlad); hipFree(p->d_ham); hipFree(p->d_knn);
  if (p->h_int) hipHostFree(p->h_int);
  if (p->h_words) hipHostFree(p->h_words);
  hipFree(p->d_ess);
  if (p->h_ess) hipHostFree(p->h_ess);
  hipFree(p->d_corr);
  if (p->h_corr) hipHostFree(p->h_corr);
  for (auto &u : p->uav_ids) delete u;
  free(p);
}

extern "C" int xk_pr_create(xk_handle *h, int k, int L, int n_nodes, int kmax, int desc_bytes,
                            const unsigned char *node_desc, const int *children, const int *word_of_node,
                            const int *node_of_word, int n_words, long payload_doubles, long tracks_doubles,
                            int max_desc, xk_pr **out) {
  if (!h || !out || !node_desc || !children || !word_of_node || !node_of_word) return XK_EINVAL;
  if (k < 1 || L < 1 || n_nodes < 2 || kmax < 1 || n_words < 1 || max_desc < 1 || payload_doubles < 0 || tracks_doubles < 0)
    return fail(h, XK_EINVAL, "xk_pr_create: bad sizes");
  if (desc_bytes < 4 || desc_bytes % 4 || desc_bytes > 4 * XK_PR_MAXW)
    return fail(h, XK_EINVAL, "xk_pr_create: descriptor size must be a multiple of 4 bytes, at most 64");
  double cl = 1.0;
  for (int i = 0; i < L; ++i) cl *= k;                       // pow(k, L), vlad.cpp:27-28
  if (cl * desc_bytes > (double)(64 << 20)) return fail(h, XK_ECAPACITY, "xk_pr_create: VLAD larger than 64 MB");
  for (int i = 0; i < n_nodes; ++i)
    if (word_of_node[i] >= n_words || word_of_node[i] >= (int)cl) return fail(h, XK_EINVAL, "xk_pr_create: word id out of range");
  xk_pr *p = (xk_pr *)calloc(1, sizeof(xk_pr));
  if (!p) return XK_ENOMEM;
  p->h = h; p->k = k; p->L = L; p->n_nodes = n_nodes; p->kmax = kmax; p->W = desc_bytes / 4; p->n_words = n_words;
  p->clusters = (int)cl; p->VW = p->clusters * p->W; p->max_desc = max_desc; p->pay_n = payload_doubles; p->trk_n = tracks_doubles;
  for (auto &u : p->uav_ids) u = new std::vector<int>();
  const size_t wcap = std::max((size_t)max_desc * p->W * 2, (size_t)p->VW * 2);
  p->h_words_cap = wcap;
  bool ok = dalloc(&p->d_node_desc, (size_t)n_nodes * p->W) == hipSuccess && dalloc(&p->d_children, (size_t)n_nodes * kmax) == hipSuccess &&
            dalloc(&p->d_word_of_node, (size_t)n_nodes) == hipSuccess && dalloc(&p->d_node_of_word, (size_t)n_words) == hipSuccess &&
            dalloc(&p->d_vlad, (size_t)XK_PR_MAX_KEYFRAMES * p->VW) == hipSuccess &&
            dalloc(&p->d_kfdesc, (size_t)XK_PR_MAX_KEYFRAMES * max_desc * p->W) == hipSuccess &&
            dalloc(&p->d_payload, (size_t)XK_PR_MAX_KEYFRAMES * payload_doubles) == hipSuccess &&
            dalloc(&p->d_tracks, (size_t)XK_PR_MAX_KEYFRAMES * tracks_doubles) == hipSuccess &&
            dalloc(&p->d_q, (size_t)max_desc * p->W) == hipSuccess && dalloc(&p->d_t, (size_t)max_desc * p->W) == hipSuccess &&
            dalloc(&p->d_qvlad, (size_t)p->VW) == hipSuccess && dalloc(&p->d_ham, (size_t)XK_PR_MAX_KEYFRAMES) == hipSuccess &&
            dalloc(&p->d_knn, (size_t)max_desc * 4) == hipSuccess &&
            hipHostMalloc((void **)&p->h_int, sizeof(int) * ((size_t)max_desc * 4 + 64)) == hipSuccess &&
            hipHostMalloc((void **)&p->h_words, sizeof(unsigned int) * wcap) == hipSuccess;
  if (ok) {
    ok = hipMemcpy(p->d_node_desc, node_desc, (size_t)n_nodes * desc_bytes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->d_children, children, sizeof(int) * (size_t)n_nodes * kmax, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->d_word_of_node, word_of_node, sizeof(int) * (size_t)n_nodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->d_node_of_word, node_of_word, sizeof(int) * (size_t)n_words, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) { xk_pr_destroy(p); return fail(h, XK_ENOMEM, "xk_pr_create: allocation failed"); }
  *out = p;
  return XK_OK;
}

extern "C" int xk_pr_vlad_bytes(const xk_pr *p) { return p ? p->VW * 4 : 0; }
extern "C" int xk_pr_size(const xk_pr *p) { return p ? p->live : 0; }

// descriptors (host) -> VLAD in `d_dst` (device); the descriptors stay in p->d_q afterwards
static int pr_vlad_device(xk_pr *p, const unsigned char *desc, int n, unsigned int *d_dst) {
  xk_handle *h = p->h;
  if (n < 0 || n > p->max_desc) return fail(h, XK_ECAPACITY, "place recognition: more descriptors than max_desc");
  HIPCHK(h, hipMemsetAsync(d_dst, 0, sizeof(unsigned int) * p->VW, h->stream));
  if (n > 0) {
    if (!desc) return fail(h, XK_EINVAL, "place recognition: null descriptors");
    memcpy(p->h_words, desc, (size_t)n * p->W * 4);
    HIPCHK(h, hipMemcpyAsync(p->d_q, p->h_words, (size_t)n * p->W * 4, hipMemcpyHostToDevice, h->stream));
    XkVladArgs a{p->d_q, n, p->W, p->d_node_desc, p->d_children, p->kmax, p->d_word_of_node, p->d_node_of_word, d_dst};
    hipLaunchKernelGGL(xk_vlad_build, dim3((n + 255) / 256), dim3(256), 0, h->stream, a);
  }
  return XK_OK;
}

extern "C" int xk_pr_compute_vlad(xk_pr *p, const unsigned char *desc, int n, unsigned char *vlad_out) {
  if (!p || !vlad_out) return XK_EINVAL;
  xk_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = pr_vlad_device(p, desc, n, p->d_qvlad);
  if (rc != XK_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(p->h_words, p->d_qvlad, sizeof(unsigned int) * p->VW, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(vlad_out, p->h_words, sizeof(unsigned int) * p->VW);
  return XK_OK;
}

extern "C" int xk_pr_add_keyframe(xk_pr *p, const unsigned char *desc, int n_desc, const double *d_payload,
                                  const double *d_tracks, long tag) {
  if (!p) return XK_EINVAL;
  xk_handle *h = p->h;
  // (checked BEFORE the oldest keyframe is dropped: a rejected call leaves the database as it was)
  if (n_desc < 0 || n_desc > p->max_desc) return fail(h, XK_ECAPACITY, "place recognition: more descriptors than max_desc");
  if (n_desc > 0 && !desc) return fail(h, XK_EINVAL, "place recognition: null descriptors");
  HIPCHK(h, hipSetDevice(h->device));
  // slot: a free one, or the oldest keyframe's (erase(begin()), database.cpp:56-58)
  int slot;
  if (p->live < XK_PR_MAX_KEYFRAMES) {
    bool used[XK_PR_MAX_KEYFRAMES] = {false};
    for (int i = 0; i < p->live; ++i) used[p->order[i]] = true;
    slot = 0;
    while (used[slot]) ++slot;
  } else {
    slot = p->order[0];
    for (int i = 1; i < p->live; ++i) p->order[i - 1] = p->order[i];
    --p->live;
  }
  int rc = pr_vlad_device(p, desc, n_desc, p->d_vlad + (size_t)slot * p->VW);
  if (rc != XK_OK) return rc;
  if (n_desc > 0)
    HIPCHK(h, hipMemcpyAsync(p->d_kfdesc + (size_t)slot * p->max_desc * p->W, p->d_q, (size_t)n_desc * p->W * 4,
                             hipMemcpyDeviceToDevice, h->stream));
  if (d_payload && p->pay_n)
    HIPCHK(h, hipMemcpyAsync(p->d_payload + (size_t)slot * p->pay_n, d_payload, sizeof(double) * p->pay_n, hipMemcpyDeviceToDevice, h->stream));
  if (d_tracks && p->trk_n)
    HIPCHK(h, hipMemcpyAsync(p->d_tracks + (size_t)slot * p->trk_n, d_tracks, sizeof(double) * p->trk_n, hipMemcpyDeviceToDevice, h->stream));
  p->n_desc[slot] = n_desc; p->tag[slot] = tag; p->uav_ids[slot]->clear();
  p->order[p->live++] = slot;
  return XK_OK;
}

extern "C" int xk_pr_find_candidate(xk_pr *p, int uav_id, const unsigned char *query_vlad, double pr_score_thr, int *index,
                                    double *score, long *tag) {
  if (!p || !query_vlad || !index) return XK_EINVAL;
  xk_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  *index = -1;
  if (score) *score = 0.0;
  if (tag) *tag = -1;
  if (p->live == 0) return XK_OK;
  memcpy(p->h_words, query_vlad, sizeof(unsigned int) * p->VW);
  HIPCHK(h, hipMemcpyAsync(p->d_qvlad, p->h_words, sizeof(unsigned int) * p->VW, hipMemcpyHostToDevice, h->stream));
  XkVladHamArgs a{p->d_qvlad, p->d_vlad, p->VW, p->d_ham};
  hipLaunchKernelGGL(xk_vlad_hamming, dim3(XK_PR_MAX_KEYFRAMES), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipMemcpyAsync(p->h_int, p->d_ham, sizeof(int) * XK_PR_MAX_KEYFRAMES, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the selection loop of Database::findCandidate (database.cpp:32-45), keyframes oldest first
  const double v_length = (double)p->VW * 32.0;
  double best = 0.0;
  int best_pos = -1;
  for (int i = 0; i < p->live; ++i) {
    const int s = p->order[i];
    bool seen = false;
    for (int u : *p->uav_ids[s]) seen |= (u == uav_id);
    if (seen) continue;
    const double sc = (v_length - (double)p->h_int[s]) / v_length;      // vlad.cpp:71
    if (sc > pr_score_thr && sc > best) { best = sc; best_pos = i; }
  }
  if (best_pos >= 0) {
    p->uav_ids[p->order[best_pos]]->push_back(uav_id);
    *index = best_pos;
    if (score) *score = best;
    if (tag) *tag = p->tag[p->order[best_pos]];
  }
  return XK_OK;
}

extern "C" int xk_pr_keyframe(xk_pr *p, int index, const double **d_payload, const double **d_tracks, int *n_desc, long *tag,
                              unsigned char *desc_out) {
  if (!p) return XK_EINVAL;
  xk_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (index < 0 || index >= p->live) return fail(h, XK_EINVAL, "xk_pr_keyframe: no such keyframe");
  const int s = p->order[index];
  if (d_payload) *d_payload = p->d_payload + (size_t)s * p->pay_n;
  if (d_tracks) *d_tracks = p->d_tracks + (size_t)s * p->trk_n;
  if (n_desc) *n_desc = p->n_desc[s];
  if (tag) *tag = p->tag[s];
  if (desc_out && p->n_desc[s] > 0) {
    HIPCHK(h, hipMemcpyAsync(p->h_words, p->d_kfdesc + (size_t)s * p->max_desc * p->W, (size_t)p->n_desc[s] * p->W * 4,
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(desc_out, p->h_words, (size_t)p->n_desc[s] * p->W * 4);
  }
  return XK_OK;
}

extern "C" int xk_pr_copy_keyframe(xk_pr *p, int index, double *d_payload_dst, double *d_tracks_dst) {
  if (!p) return XK_EINVAL;
  xk_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (index < 0 || index >= p->live) return fail(h, XK_EINVAL, "xk_pr_copy_keyframe: no such keyframe");
  const int s = p->order[index];
  if (d_payload_dst && p->pay_n)
    HIPCHK(h, hipMemcpyAsync(d_payload_dst, p->d_payload + (size_t)s * p->pay_n, sizeof(double) * p->pay_n, hipMemcpyDeviceToDevice, h->stream));
  if (d_tracks_dst && p->trk_n)
    HIPCHK(h, hipMemcpyAsync(d_tracks_dst, p->d_tracks + (size_t)s * p->trk_n, sizeof(double) * p->trk_n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return XK_OK;
}

extern "C" int xk_pr_knn_match(xk_pr *p, const unsigned char *query, int nq, const unsigned char *train, int nt, int *idx,
                               int *dist) {
  if (!p || !idx || !dist || nq < 0 || nt < 0) return XK_EINVAL;
  xk_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (nq > p->max_desc || nt > p->max_desc) return fail(h, XK_ECAPACITY, "xk_pr_knn_match: more descriptors than max_desc");
  if (nq == 0) return XK_OK;
  if (!query || (nt > 0 && !train)) return fail(h, XK_EINVAL, "xk_pr_knn_match: null descriptors");
  const size_t qb = (size_t)nq * p->W * 4, tb = (size_t)nt * p->W * 4;
  memcpy(p->h_words, query, qb);
  if (nt) memcpy(p->h_words + (size_t)nq * p->W, train, tb);
  HIPCHK(h, hipMemcpyAsync(p->d_q, p->h_words, qb, hipMemcpyHostToDevice, h->stream));
  if (nt) HIPCHK(h, hipMemcpyAsync(p->d_t, p->h_words + (size_t)nq * p->W, tb, hipMemcpyHostToDevice, h->stream));
  XkKnnArgs a{p->d_q, p->d_t, nq, nt, p->W, p->d_knn, p->d_knn + 2 * (size_t)p->max_desc};
  hipLaunchKernelGGL(xk_desc_knn2, dim3((nq + XK_KNN_Q - 1) / XK_KNN_Q), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipMemcpyAsync(p->h_int, p->d_knn, sizeof(int) * 2 * (size_t)nq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->h_int + 2 * (size_t)nq, p->d_knn + 2 * (size_t)p->max_desc, sizeof(int) * 2 * (size_t)nq,
                           hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(idx, p->h_int, sizeof(int) * 2 * (size_t)nq);
  memcpy(dist, p->h_int + 2 * (size_t)nq, sizeof(int) * 2 * (size_t)nq);
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Essential-matrix RANSAC filter of findCorrespondences (place_recognition.cpp:269-281), xk_essential.hip.h
// ---------------------------------------------------------------------------
static XkEssArgs ess_args(xk_pr *p) {
  XkEssArgs a{};
  a.s = xk_ransac_scratch<XK_ESS_MAXC>(p->d_ess, XK_ESS_MAX_HYP);
  a.E = (double *)(p->d_ess + xk_ransac_scratch_bytes<XK_ESS_MAXC>(XK_ESS_MAX_HYP));   // (a multiple of 8)
  a.res = (int *)(a.E + 9);
  float *xy = (float *)(a.res + 2);
  a.cur_xy = xy;                                             // (rec_xy follows the n pairs of the call)
  a.mask = (unsigned char *)(xy + 4 * (size_t)p->max_desc);
  return a;
}

static size_t ess_xy_bytes(const xk_pr *p) { return sizeof(float) * 4 * (size_t)p->max_desc; }
static size_t ess_out_bytes(const xk_pr *p) { return 9 * sizeof(double) + 2 * sizeof(int) + (size_t)p->max_desc; }

// the essential block and its pinned mirror, on first use
static int ess_reserve(xk_pr *p) {
  if (p->d_ess) return XK_OK;
  xk_handle *h = p->h;
  void *d = nullptr, *hp = nullptr;
  if (hipMalloc(&d, xk_ransac_scratch_bytes<XK_ESS_MAXC>(XK_ESS_MAX_HYP) + ess_xy_bytes(p) + ess_out_bytes(p)) != hipSuccess)
    return fail(h, XK_ENOMEM, "xk_pr_essential_ransac: scratch block");
  if (hipHostMalloc(&hp, ess_xy_bytes(p) + ess_out_bytes(p)) != hipSuccess) { hipFree(d); return fail(h, XK_ENOMEM, "xk_pr_essential_ransac: pinned block"); }
  p->d_ess = (unsigned char *)d;
  p->h_ess = (unsigned char *)hp;
  return XK_OK;
}

extern "C" int xk_pr_essential_ransac(xk_pr *p, const float *cur_xy, const float *rec_xy, int n, double fx, double fy, double cx,
                                      double cy, double threshold_px, int n_hyp, unsigned long seed, unsigned char *mask,
                                      double *E, int *n_inliers) {
  if (!p) return XK_EINVAL;
  xk_handle *h = p->h;
  if (!mask || !n_inliers || n < 0 || (n > 0 && (!cur_xy || !rec_xy)))
    return fail(h, XK_EINVAL, "xk_pr_essential_ransac: null argument or negative n");
  if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
    return fail(h, XK_EINVAL, "xk_pr_essential_ransac: focal lengths must be positive and the intrinsics finite");
  if (!(threshold_px >= 0.0) || !std::isfinite(threshold_px)) return fail(h, XK_EINVAL, "xk_pr_essential_ransac: threshold_px < 0");
  if (n_hyp < 1 || n_hyp > XK_ESS_MAX_HYP) return fail(h, XK_EINVAL, "xk_pr_essential_ransac: n_hyp outside 1...4096");
  if (n > p->max_desc) return fail(h, XK_ECAPACITY, "xk_pr_essential_ransac: more point pairs than max_desc");
  *n_inliers = 0;
  memset(mask, 0, (size_t)n);
  if (E) memset(E, 0, 9 * sizeof(double));
  if (n < 5) return XK_OK;                                   // F_1.empty() -> return false
  HIPCHK(h, hipSetDevice(h->device));
  const size_t xy_bytes = ess_xy_bytes(p), out_bytes = ess_out_bytes(p);
  const int rc = ess_reserve(p);
  if (rc != XK_OK) return rc;
  XkEssArgs a = ess_args(p);
  a.n = n; a.n_hyp = n_hyp;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  const double t = threshold_px / ((fx + fy) / 2.0);
  a.t2 = t * t;
  a.seed = (unsigned long long)seed;
  float *h_xy = (float *)p->h_ess;                           // cur [n][2], then rec [n][2] right behind it: one copy of 4n floats
  memcpy(h_xy, cur_xy, sizeof(float) * 2 * (size_t)n);
  memcpy(h_xy + 2 * (size_t)n, rec_xy, sizeof(float) * 2 * (size_t)n);
  a.rec_xy = a.cur_xy + 2 * (size_t)n;
  p->ess_n_hyp = 0;
  HIPCHK(h, hipMemcpyAsync((void *)a.cur_xy, h_xy, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(xk_ess_solve, dim3((n_hyp + XK_ESS_SOLVE_T - 1) / XK_ESS_SOLVE_T), dim3(XK_ESS_SOLVE_T), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ess_score, dim3(n_hyp), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ess_mask, dim3((n + 255) / 256), dim3(256), 0, h->stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, XK_EDEVICE, "essential RANSAC launch", e);
  unsigned char *h_out = p->h_ess + xy_bytes;                // E [9] | n_inliers, winner | mask [n]
  HIPCHK(h, hipMemcpyAsync(h_out, a.E, 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h_out + 9 * sizeof(double), a.res, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h_out + 9 * sizeof(double) + 2 * sizeof(int), a.mask, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  p->ess_n_hyp = n_hyp;
  if (E) memcpy(E, h_out, 9 * sizeof(double));
  memcpy(n_inliers, h_out + 9 * sizeof(double), sizeof(int));
  memcpy(mask, h_out + 9 * sizeof(double) + 2 * sizeof(int), (size_t)n);
  return XK_OK;
}

extern "C" int xk_pr_essential_hypotheses(xk_pr *p, int first, int count, int *n_cand, double *E, int *inliers) {
  if (!p) return XK_EINVAL;
  return ransac_hypotheses(p->h, "xk_pr_essential_hypotheses", "xk_pr_essential_ransac", p->d_ess ? p->ess_n_hyp : -1,
                           p->d_ess ? ess_args(p).s : XkRansacScratch{}, XK_ESS_MAXC, first, count, n_cand, E, inliers);
}

// ---------------------------------------------------------------------------
// findCorrespondences in one call (place_recognition.cpp:137-385, the non-GT branch), xk_correspond.hip.h: one copy in, six
// launches with the candidate count in device memory, one result block out, one wait
// ---------------------------------------------------------------------------
// The result block for the bound n: head | E [9] | good [n][2] | classified [n][3] | candidates [n][2] | remove_ids [n] | mask [n]
struct XkCorrResult {
  XkCorrHead *head;
  double *E;
  int *good, *classified, *cand, *remove_ids;
  unsigned char *mask;
};
static size_t corr_result_bytes(size_t n) { return sizeof(XkCorrHead) + 9 * sizeof(double) + sizeof(int) * 8 * n + n; }
static XkCorrResult corr_result(unsigned char *at, size_t n) {   // at: 8-byte aligned
  XkCorrResult r;
  r.head = (XkCorrHead *)at;
  r.E = (double *)(r.head + 1);
  r.good = (int *)(r.E + 9); r.classified = r.good + 2 * n; r.cand = r.classified + 3 * n; r.remove_ids = r.cand + 2 * n;
  r.mask = (unsigned char *)(r.remove_ids + n);
  return r;
}
// the device block: input (descriptors and pixels of both sides, packed by the call's counts) | alive | G | first_j | count | result
static size_t corr_in_bytes(const xk_pr *p) { return (size_t)p->max_desc * (8 * (size_t)p->W + 16); }   // (a multiple of 8)
static size_t corr_work_bytes(const xk_pr *p) {
  const size_t M = (size_t)p->max_desc;
  return (8 * ((M + 63) / 64) + sizeof(int) * (3 * M + 2) + 7) / 8 * 8;
}

extern "C" int xk_pr_find_correspondences(xk_pr *p, const unsigned char *rec_desc, const float *rec_xy, int n_rec,
                                          const unsigned char *cur_desc, const float *cur_xy, int n_cur, int n_cur_msckf,
                                          int n_cur_slam, int n_rec_msckf, int n_rec_slam, double pr_min_distance,
                                          double pr_ratio_thr, double fx, double fy, double cx, double cy, double threshold_px,
                                          int n_hyp, unsigned long seed, xk_pr_corr_out *out, int *good, int *classified) {
  if (!p) return XK_EINVAL;
  xk_handle *h = p->h;
  if (!out || n_rec < 0 || n_cur < 0 || (n_rec > 0 && (!rec_desc || !rec_xy)) || (n_cur > 0 && (!cur_desc || !cur_xy)))
    return fail(h, XK_EINVAL, "xk_pr_find_correspondences: null argument or negative count");
  if (n_cur_msckf < 0 || n_cur_slam < 0 || n_rec_msckf < 0 || n_rec_slam < 0 || (long)n_cur_msckf + n_cur_slam > n_cur ||
      (long)n_rec_msckf + n_rec_slam > n_rec)
    return fail(h, XK_EINVAL, "xk_pr_find_correspondences: class counts negative or beyond their side");
  if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
    return fail(h, XK_EINVAL, "xk_pr_find_correspondences: focal lengths must be positive and the intrinsics finite");
  if (!(threshold_px >= 0.0) || !std::isfinite(threshold_px)) return fail(h, XK_EINVAL, "xk_pr_find_correspondences: threshold_px < 0");
  if (n_hyp < 1 || n_hyp > XK_ESS_MAX_HYP) return fail(h, XK_EINVAL, "xk_pr_find_correspondences: n_hyp outside 1...4096");
  if (n_rec > p->max_desc || n_cur > p->max_desc) return fail(h, XK_ECAPACITY, "xk_pr_find_correspondences: more descriptors than max_desc");
  memset(out, 0, sizeof(*out));
  out->winner = -1;
  p->corr_called = true;
  p->corr_n_rec = -1;
  if (n_cur == 0 || n_rec == 0) {                            // :209, :244 -- decided here, nothing queued
    out->status = n_cur == 0 ? 1 : 2;
    p->corr_n_rec = 0;
    return XK_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = ess_reserve(p);
  if (rc != XK_OK) return rc;
  const size_t in_cap = corr_in_bytes(p), work = corr_work_bytes(p), res_cap = corr_result_bytes((size_t)p->max_desc);
  if (!p->d_corr) {
    void *d = nullptr, *hp = nullptr;
    if (hipMalloc(&d, in_cap + work + res_cap) != hipSuccess) return fail(h, XK_ENOMEM, "xk_pr_find_correspondences: device block");
    if (hipHostMalloc(&hp, in_cap + res_cap) != hipSuccess) { hipFree(d); return fail(h, XK_ENOMEM, "xk_pr_find_correspondences: pinned block"); }
    p->d_corr = (unsigned char *)d;
    p->h_corr = (unsigned char *)hp;
  }
  // one pinned block, one copy: received descriptors | current descriptors | received pixels | current pixels
  const size_t W = (size_t)p->W, rdb = (size_t)n_rec * W * 4, cdb = (size_t)n_cur * W * 4, rxb = sizeof(float) * 2 * (size_t)n_rec,
               cxb = sizeof(float) * 2 * (size_t)n_cur;
  memcpy(p->h_corr, rec_desc, rdb);
  memcpy(p->h_corr + rdb, cur_desc, cdb);
  memcpy(p->h_corr + rdb + cdb, rec_xy, rxb);
  memcpy(p->h_corr + rdb + cdb + rxb, cur_xy, cxb);
  HIPCHK(h, hipMemcpyAsync(p->d_corr, p->h_corr, rdb + cdb + rxb + cxb, hipMemcpyHostToDevice, h->stream));
  const unsigned int *d_rec_desc = (const unsigned int *)p->d_corr, *d_cur_desc = (const unsigned int *)(p->d_corr + rdb);
  const float *d_rec_xy = (const float *)(p->d_corr + rdb + cdb), *d_cur_xy = (const float *)(p->d_corr + rdb + cdb + rxb);
  unsigned long long *d_alive = (unsigned long long *)(p->d_corr + in_cap);
  int *d_G = (int *)(d_alive + ((size_t)p->max_desc + 63) / 64), *d_fj = d_G + 2 * (size_t)p->max_desc, *d_count = d_fj + p->max_desc;
  const XkCorrResult R = corr_result(p->d_corr + in_cap + work, (size_t)n_rec);

  XkKnnArgs ka{d_rec_desc, d_cur_desc, n_rec, n_cur, p->W, p->d_knn, p->d_knn + 2 * (size_t)p->max_desc};
  hipLaunchKernelGGL(xk_desc_knn2, dim3((n_rec + XK_KNN_Q - 1) / XK_KNN_Q), dim3(256), 0, h->stream, ka);
  XkEssArgs a = ess_args(p);
  a.rec_xy = a.cur_xy + 2 * (size_t)p->max_desc;             // (the stage entry packs it 2 n behind; here n is on the device)
  a.n = n_rec; a.n_dev = d_count; a.n_hyp = n_hyp;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  const double t = threshold_px / ((fx + fy) / 2.0);
  a.t2 = t * t;
  a.seed = (unsigned long long)seed;
  XkCorrCandArgs ca{ka.idx, ka.dist, n_rec, pr_min_distance, pr_ratio_thr, d_rec_xy, d_cur_xy, (float *)a.cur_xy, (float *)a.rec_xy,
                    R.cand, d_count};
  hipLaunchKernelGGL(xk_corr_candidates, dim3(1), dim3(256), 0, h->stream, ca);
  p->ess_n_hyp = 0;
  hipLaunchKernelGGL(xk_ess_solve, dim3((n_hyp + XK_ESS_SOLVE_T - 1) / XK_ESS_SOLVE_T), dim3(XK_ESS_SOLVE_T), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ess_score, dim3(n_hyp), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(xk_ess_mask, dim3((n_rec + 255) / 256), dim3(256), 0, h->stream, a);
  XkCorrFinishArgs fa{n_rec, d_count, R.cand, a.mask, a.E, a.res, n_cur_msckf, n_cur_slam, n_rec_msckf, n_rec_slam, d_G, d_fj, d_alive,
                      R.head, R.E, R.good, R.classified, R.remove_ids, R.mask};
  hipLaunchKernelGGL(xk_corr_finish, dim3(1), dim3(256), 0, h->stream, fa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, XK_EDEVICE, "xk_pr_find_correspondences launch", e);
  unsigned char *h_res = p->h_corr + in_cap;
  HIPCHK(h, hipMemcpyAsync(h_res, R.head, corr_result_bytes((size_t)n_rec), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  p->ess_n_hyp = n_hyp;
  p->corr_n_rec = n_rec;
  const XkCorrResult H = corr_result(h_res, (size_t)n_rec);
  out->status = H.head->status; out->n_candidates = H.head->n_candidates; out->n_inliers = H.head->n_inliers;
  out->winner = H.head->winner; out->n_good = H.head->n_good; out->n_classified = H.head->n_classified;
  out->launches = 6;
  memcpy(out->E, H.E, 9 * sizeof(double));
  if (good) memcpy(good, H.good, sizeof(int) * 2 * (size_t)out->n_good);
  if (classified) memcpy(classified, H.classified, sizeof(int) * 3 * (size_t)out->n_classified);
  return XK_OK;
}

extern "C" int xk_pr_find_correspondences_stage(xk_pr *p, int *candidates, unsigned char *mask, int *remove_ids, int *n_remove) {
  if (!p) return XK_EINVAL;
  xk_handle *h = p->h;
  if (!p->corr_called || p->corr_n_rec < 0) return fail(h, XK_EINVAL, "xk_pr_find_correspondences_stage: no completed xk_pr_find_correspondences");
  if (n_remove) *n_remove = 0;
  if (p->corr_n_rec == 0) return XK_OK;                      // (statuses 1 and 2: nothing was queued)
  const size_t n = (size_t)p->corr_n_rec;
  const XkCorrResult H = corr_result(p->h_corr + corr_in_bytes(p), n);
  if (candidates) memcpy(candidates, H.cand, sizeof(int) * 2 * (size_t)H.head->n_candidates);
  if (mask) memcpy(mask, H.mask, n);
  if (remove_ids) memcpy(remove_ids, H.remove_ids, sizeof(int) * (size_t)H.head->n_remove);
  if (n_remove) *n_remove = H.head->n_remove;
  return XK_OK;
}

// ---------------------------------------------------------------------------
// Vocabulary training (DBoW3::Vocabulary::create, third_party/DBow3/src/Vocabulary.cpp:157-186), xk_vocab.hip.h
// ---------------------------------------------------------------------------
struct XkVocHostNode { int first_child, nchild; };   // a node's children are one block of the host list

struct xk_voc {
  xk_handle *h;
  int k, L, W, max_desc, count;
  unsigned int *d_desc;                 // [max_desc][W]
  int *d_perm[2], *d_nop[2];            // this level's and the next level's permutation / node of every position
  int *d_assoc, *d_min, *d_hist;
  unsigned long long *d_prefix, *d_bsum, *d_rec;
  // sized by the nodes of a level, grown between levels
  size_t a_cap;
  XkVocNode *d_nodes;
  unsigned int *d_cen;
  int *d_cnt, *d_gsize, *d_csize, *d_dstoff, *d_childnext;
  unsigned char *h_pin;                 // pinned: nodes | centres | csize | dst_off | child_next, each for a_cap nodes
  unsigned long long *h_rec;            // pinned record: nodes that went on, capped nodes, changed associations (cumulative)
  // the trained tree, DBoW3 order
  bool trained;
  std::vector<unsigned int> r_desc;
  std::vector<int> r_children, r_won, r_now;
  xk_voc_outcome outcome;
};

static void voc_free_level(xk_voc *v) {
  hipFree(v->d_nodes); hipFree(v->d_cen); hipFree(v->d_cnt); hipFree(v->d_gsize); hipFree(v->d_csize); hipFree(v->d_dstoff);
  hipFree(v->d_childnext);
  if (v->h_pin) hipHostFree(v->h_pin);
  v->d_nodes = nullptr; v->d_cen = nullptr; v->d_cnt = v->d_gsize = v->d_csize = v->d_dstoff = v->d_childnext = nullptr;
  v->h_pin = nullptr; v->a_cap = 0;
}

extern "C" void xk_voc_destroy(xk_voc *v) {
  if (!v) return;
  hipFree(v->d_desc); hipFree(v->d_perm[0]); hipFree(v->d_perm[1]); hipFree(v->d_nop[0]); hipFree(v->d_nop[1]);
  hipFree(v->d_assoc); hipFree(v->d_min); hipFree(v->d_hist); hipFree(v->d_prefix); hipFree(v->d_bsum); hipFree(v->d_rec);
  voc_free_level(v);
  if (v->h_rec) hipHostFree(v->h_rec);
  delete v;
}

extern "C" int xk_voc_create(xk_handle *h, int k, int L, int desc_bytes, int max_desc, xk_voc **out) {
  if (!h || !out) return XK_EINVAL;
  if (k < 2 || k > XK_VOC_KMAX || L < 1 || L > XK_VOC_LMAX || max_desc < 1) return fail(h, XK_EINVAL, "xk_voc_create: k outside 2...16, L outside 1...8 or max_desc < 1");
  if (desc_bytes < 4 || desc_bytes % 4 || desc_bytes > 4 * XK_PR_MAXW)
    return fail(h, XK_EINVAL, "xk_voc_create: descriptor size must be a multiple of 4 bytes, at most 64");
  double cl = 1.0;
  for (int i = 0; i < L; ++i) cl *= k;
  if (cl * desc_bytes > (double)(64 << 20)) return fail(h, XK_ECAPACITY, "xk_voc_create: k^L descriptors larger than 64 MB");
  HIPCHK(h, hipSetDevice(h->device));
  xk_voc *v = new (std::nothrow) xk_voc();
  if (!v) return XK_ENOMEM;
  v->h = h; v->k = k; v->L = L; v->W = desc_bytes / 4; v->max_desc = max_desc;
  const size_t nb = ((size_t)max_desc + XK_VOC_T - 1) / XK_VOC_T;
  const bool ok = dalloc(&v->d_desc, (size_t)max_desc * v->W) == hipSuccess && dalloc(&v->d_perm[0], (size_t)max_desc) == hipSuccess &&
                  dalloc(&v->d_perm[1], (size_t)max_desc) == hipSuccess && dalloc(&v->d_nop[0], (size_t)max_desc) == hipSuccess &&
                  dalloc(&v->d_nop[1], (size_t)max_desc) == hipSuccess && dalloc(&v->d_assoc, (size_t)max_desc) == hipSuccess &&
                  dalloc(&v->d_min, (size_t)max_desc) == hipSuccess && dalloc(&v->d_prefix, (size_t)max_desc) == hipSuccess &&
                  dalloc(&v->d_bsum, nb) == hipSuccess && dalloc(&v->d_hist, nb * k) == hipSuccess && dalloc(&v->d_rec, (size_t)4) == hipSuccess &&
                  hipHostMalloc((void **)&v->h_rec, 4 * sizeof(unsigned long long)) == hipSuccess;
  if (!ok) { xk_voc_destroy(v); return fail(h, XK_ENOMEM, "xk_voc_create: allocation failed"); }
  *out = v;
  return XK_OK;
}

extern "C" int xk_voc_count(const xk_voc *v) { return v ? v->count : 0; }

extern "C" int xk_voc_clear(xk_voc *v) {
  if (!v) return XK_EINVAL;
  v->count = 0;
  v->trained = false;
  return XK_OK;
}

extern "C" int xk_voc_add(xk_voc *v, const unsigned char *desc, int n) {
  if (!v) return XK_EINVAL;
  xk_handle *h = v->h;
  if (n < 0 || (n > 0 && !desc)) return fail(h, XK_EINVAL, "xk_voc_add: n < 0 or null descriptors");
  if (n > v->max_desc - v->count) return fail(h, XK_ECAPACITY, "xk_voc_add: more descriptors than max_desc");
  if (n == 0) return XK_OK;
  HIPCHK(h, hipSetDevice(h->device));
  // (the caller's rows are pageable: the copy is staged by the runtime, and the wait makes the rows the caller's again)
  HIPCHK(h, hipMemcpyAsync(v->d_desc + (size_t)v->count * v->W, desc, (size_t)n * v->W * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  v->count += n;
  return XK_OK;
}

// the pinned block (the nodes first, then the regions below) and the device buffers for levels of up to `a` nodes; the
// stream is idle when voc_reserve is called
static size_t voc_pin_cen(size_t cap) { return sizeof(XkVocNode) * cap; }
static size_t voc_pin_csize(const xk_voc *v, size_t cap) { return voc_pin_cen(cap) + sizeof(int) * cap * v->k * v->W; }
static size_t voc_pin_dstoff(const xk_voc *v, size_t cap) { return voc_pin_csize(v, cap) + sizeof(int) * cap * v->k; }
static size_t voc_pin_childnext(const xk_voc *v, size_t cap) { return voc_pin_dstoff(v, cap) + sizeof(int) * cap * v->k; }
static size_t voc_pin_bytes(const xk_voc *v, size_t cap) { return voc_pin_childnext(v, cap) + sizeof(int) * cap * v->k; }

static int voc_reserve(xk_voc *v, size_t a) {
  if (a <= v->a_cap) return XK_OK;
  xk_handle *h = v->h;
  voc_free_level(v);
  const size_t cap = std::max(a, (size_t)64), g = cap * v->k;
  const bool ok = dalloc(&v->d_nodes, cap) == hipSuccess && dalloc(&v->d_cen, g * v->W) == hipSuccess &&
                  dalloc(&v->d_cnt, g * v->W * 32) == hipSuccess && dalloc(&v->d_gsize, g) == hipSuccess &&
                  dalloc(&v->d_csize, g) == hipSuccess && dalloc(&v->d_dstoff, g) == hipSuccess && dalloc(&v->d_childnext, g) == hipSuccess &&
                  hipHostMalloc((void **)&v->h_pin, voc_pin_bytes(v, cap)) == hipSuccess;
  if (!ok) { voc_free_level(v); return fail(h, XK_ENOMEM, "xk_voc_train: buffers of a level"); }
  v->a_cap = cap;
  HIPCHK(h, hipMemsetAsync(v->d_cnt, 0, sizeof(int) * g * v->W * 32, h->stream));   // (the majority kernels leave it zero)
  return XK_OK;
}

extern "C" int xk_voc_train(xk_voc *v, unsigned long seed, int max_iter, xk_voc_outcome *outcome) {
  if (!v) return XK_EINVAL;
  xk_handle *h = v->h;
  if (max_iter < 1) return fail(h, XK_EINVAL, "xk_voc_train: max_iter < 1");
  HIPCHK(h, hipSetDevice(h->device));
  v->trained = false;
  const int k = v->k, W = v->W, N = v->count;
  xk_voc_outcome oc{};
  struct Lv { int start, cnt, hid; unsigned long long path; };
  std::vector<Lv> cur, nxt;
  std::vector<XkVocHostNode> hn(1, XkVocHostNode{0, 0});   // host list, level order; [0] is the root
  std::vector<unsigned int> hdesc((size_t)W, 0u);          // [host node][W]
  const dim3 T(XK_VOC_T);
  auto blocks = [](size_t n) { return dim3((unsigned int)((n + XK_VOC_T - 1) / XK_VOC_T)); };
  int which = 0, M = N;
  unsigned long long went_on = 0;
  if (N > 0) {
    int rc = voc_reserve(v, 1);
    if (rc != XK_OK) return rc;
    HIPCHK(h, hipMemsetAsync(v->d_rec, 0, 4 * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(xk_voc_iota, blocks(N), T, 0, h->stream, v->d_perm[0], v->d_nop[0], N);
    ++oc.launches;
    cur.push_back(Lv{0, N, 0, 0ull});
  }
  for (int level = 1; level <= v->L && !cur.empty(); ++level) {
    const int A = (int)cur.size();
    const size_t cap = v->a_cap;
    XkVocNode *pn = (XkVocNode *)v->h_pin;
    bool nontrivial = false;
    for (int a = 0; a < A; ++a) {
      pn[a] = XkVocNode{cur[a].start, cur[a].cnt, 0, cur[a].cnt > k ? 1 : 0, 0, 0,
                        xk_ransac_mix((unsigned long long)seed ^ xk_ransac_mix(cur[a].path))};
      nontrivial |= cur[a].cnt > k;
    }
    HIPCHK(h, hipMemcpyAsync(v->d_nodes, pn, sizeof(XkVocNode) * A, hipMemcpyHostToDevice, h->stream));
    XkVocLevel lv{v->d_desc, W, k, M, A, v->d_perm[which], v->d_nop[which], v->d_nodes, v->d_cen, v->d_assoc, v->d_min,
                  v->d_prefix, v->d_bsum, v->d_cnt, v->d_gsize, v->d_csize, v->d_hist, v->d_rec};
    const dim3 GM = blocks(M), GA = blocks(A);
    hipLaunchKernelGGL(xk_voc_seed_first, GA, T, 0, h->stream, lv);
    ++oc.launches;
    int passes = 0;
    if (nontrivial) {
      for (int j = 1; j < k; ++j) {                          // the cut is formed on the device: no wait while seeding
        hipLaunchKernelGGL(xk_voc_seed_dist, GM, T, 0, h->stream, lv, j);
        hipLaunchKernelGGL(xk_voc_scan_u64, dim3(1), T, 0, h->stream, v->d_bsum, (int)GM.x);
        hipLaunchKernelGGL(xk_voc_prefix, GM, T, 0, h->stream, lv);
        hipLaunchKernelGGL(xk_voc_seed_pick, GM, T, 0, h->stream, lv, j);
        oc.launches += 4;
      }
      for (int pass = 1;; ++pass) {
        hipLaunchKernelGGL(xk_voc_assoc, GM, T, 0, h->stream, lv, pass);
        hipLaunchKernelGGL(xk_voc_status, GA, T, 0, h->stream, lv, pass, max_iter);
        oc.launches += 2;
        HIPCHK(h, hipMemcpyAsync(v->h_rec, v->d_rec, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        if (pass < max_iter) {                               // queued before the wait: nothing to do where no node goes on
          hipLaunchKernelGGL(xk_voc_majority_count, GM, T, 0, h->stream, lv);
          hipLaunchKernelGGL(xk_voc_majority_set, blocks((size_t)A * k * W), T, 0, h->stream, lv);
          oc.launches += 2;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        ++oc.host_waits;
        passes = pass;
        const bool more = v->h_rec[0] != went_on;
        went_on = v->h_rec[0];
        oc.capped_nodes = (int)v->h_rec[1];
        if (!more) break;
      }
    }
    // the level's result: children and centres of every node, and (above the last level) the sizes of the groups
    int *pcs = (int *)(v->h_pin + voc_pin_csize(v, cap));
    unsigned int *pcen = (unsigned int *)(v->h_pin + voc_pin_cen(cap));
    const bool split = level < v->L;
    if (split) {
      HIPCHK(h, hipMemsetAsync(v->d_csize, 0, sizeof(int) * (size_t)A * k, h->stream));
      hipLaunchKernelGGL(xk_voc_hist, GM, T, 0, h->stream, lv);
      hipLaunchKernelGGL(xk_voc_scan_hist, dim3(1), T, 0, h->stream, v->d_hist, (int)GM.x, k);
      oc.launches += 2;
      HIPCHK(h, hipMemcpyAsync(pcs, v->d_csize, sizeof(int) * (size_t)A * k, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(pn, v->d_nodes, sizeof(XkVocNode) * A, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(pcen, v->d_cen, sizeof(int) * (size_t)A * k * W, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ++oc.host_waits;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, XK_EDEVICE, "xk_voc_train launch", e);
    oc.level_nodes[level - 1] = A;
    oc.level_passes[level - 1] = passes;
    oc.levels = level;
    // host walk: one host node per centre; a child with more than one descriptor is a node of the next level (:371-392)
    nxt.clear();
    std::vector<int> dst_off((size_t)A * k, 0), child_next((size_t)A * k, -1);
    int cum[XK_VOC_KMAX] = {0};
    int M_next = 0;
    for (int a = 0; a < A; ++a) {
      const int nc = pn[a].ncent;
      if (nc < 1 || nc > k) return fail(h, XK_EDEVICE, "xk_voc_train: a node without centres");
      hn[cur[a].hid] = XkVocHostNode{(int)hn.size(), nc};
      for (int c = 0; c < nc; ++c) {
        const int id = (int)hn.size();
        hn.push_back(XkVocHostNode{0, 0});
        hdesc.insert(hdesc.end(), pcen + ((size_t)a * k + c) * W, pcen + ((size_t)a * k + c + 1) * W);
        if (split) {
          const int sz = pcs[(size_t)a * k + c];
          if (sz > 1) {
            child_next[(size_t)a * k + c] = (int)nxt.size();
            dst_off[(size_t)a * k + c] = M_next - cum[c];
            nxt.push_back(Lv{M_next, sz, id, cur[a].path * (unsigned long long)(k + 1) + (unsigned long long)c + 1ull});
            M_next += sz;
          }
          cum[c] += sz;
        }
      }
    }
    if (!nxt.empty()) {
      int rc = voc_reserve(v, std::max(nxt.size(), (size_t)A));   // (may move the pinned block: pn, pcs, pcen end here)
      if (rc != XK_OK) return rc;
      int *pdo = (int *)(v->h_pin + voc_pin_dstoff(v, v->a_cap)), *pch = (int *)(v->h_pin + voc_pin_childnext(v, v->a_cap));
      memcpy(pdo, dst_off.data(), sizeof(int) * (size_t)A * k);
      memcpy(pch, child_next.data(), sizeof(int) * (size_t)A * k);
      HIPCHK(h, hipMemcpyAsync(v->d_dstoff, pdo, sizeof(int) * (size_t)A * k, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(v->d_childnext, pch, sizeof(int) * (size_t)A * k, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemsetAsync(v->d_nop[which ^ 1], 0xff, sizeof(int) * (size_t)M_next, h->stream));   // (-1: no node)
      hipLaunchKernelGGL(xk_voc_scatter, GM, T, 0, h->stream, lv, (const int *)v->d_dstoff, (const int *)v->d_childnext,
                         v->d_perm[which ^ 1], v->d_nop[which ^ 1], M_next);
      ++oc.launches;
      which ^= 1;
      M = M_next;
    }
    cur.swap(nxt);
  }
  // DBoW3's ids: a node's children are appended as one block, then the recursion descends into them in order (:361-393)
  const int n_nodes = (int)hn.size();
  std::vector<int> newid((size_t)n_nodes, 0);
  int next_id = 1;
  std::function<void(int)> walk = [&](int id) {
    for (int c = 0; c < hn[id].nchild; ++c) newid[hn[id].first_child + c] = next_id++;
    for (int c = 0; c < hn[id].nchild; ++c)
      if (hn[hn[id].first_child + c].nchild) walk(hn[id].first_child + c);
  };
  walk(0);
  v->r_desc.assign((size_t)n_nodes * W, 0u);
  v->r_children.assign((size_t)n_nodes * k, -1);
  v->r_won.assign((size_t)n_nodes, -1);
  std::vector<int> old_of_new((size_t)n_nodes, 0);
  for (int id = 0; id < n_nodes; ++id) {
    const int ni = newid[id];
    old_of_new[ni] = id;
    memcpy(&v->r_desc[(size_t)ni * W], &hdesc[(size_t)id * W], sizeof(unsigned int) * W);
    for (int c = 0; c < hn[id].nchild; ++c) v->r_children[(size_t)ni * k + c] = newid[hn[id].first_child + c];
  }
  v->r_now.clear();
  for (int ni = 1; ni < n_nodes; ++ni)                       // createWords (:496-515): the leaves in id order, root excluded
    if (hn[old_of_new[ni]].nchild == 0) {
      v->r_won[ni] = (int)v->r_now.size();
      v->r_now.push_back(ni);
    }
  oc.n_nodes = n_nodes;
  oc.n_words = (int)v->r_now.size();
  v->outcome = oc;
  v->trained = true;
  if (outcome) *outcome = oc;
  return XK_OK;
}

extern "C" int xk_voc_get(const xk_voc *v, unsigned char *node_desc, int *children, int *word_of_node, int *node_of_word) {
  if (!v) return XK_EINVAL;
  if (!v->trained) return fail(v->h, XK_EINVAL, "xk_voc_get: no trained tree");
  if (node_desc) memcpy(node_desc, v->r_desc.data(), sizeof(unsigned int) * v->r_desc.size());
  if (children) memcpy(children, v->r_children.data(), sizeof(int) * v->r_children.size());
  if (word_of_node) memcpy(word_of_node, v->r_won.data(), sizeof(int) * v->r_won.size());
  if (node_of_word && !v->r_now.empty()) memcpy(node_of_word, v->r_now.data(), sizeof(int) * v->r_now.size());
  return XK_OK;
}
