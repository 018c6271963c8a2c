// The non-GT branch of PlaceRecognition::findCorrespondences (place_recognition.cpp:249-388) end to end on the mirror,
// from a text case file (written by tests/test_gpu_correspondences_host.py), one printed line per stage.
//   header : desc_bytes min_distance ratio fx fy cx cy threshold n_hyp seed
//   sizes  : n_rec n_cur n_cur_msckf n_cur_slam n_rec_msckf n_rec_slam
//   arrays : received descriptors, received pixels (x y per row), current descriptors, current pixels
//   output : K <idx0:dist0:idx1:dist1 per received row>      knnMatch
//            G <q:t ...>                                     goodMatches without a mask (the points come from these)
//            E <n_inliers> <mask bits>                       essentialInliers
//            F <q:t ...>                                     goodMatches with the mask
//            C <kind:current:received ...>                   classifyMatches
#include <cstdio>
#include <fstream>
#include <iostream>

#include "x/place_recognition/database.h"

using namespace x;

static Descriptors readDesc(std::istream &in, int rows, int cols) {
  Descriptors d;
  d.rows = rows; d.cols = cols;
  d.data.resize((size_t)rows * cols);
  for (auto &b : d.data) { int v; in >> v; b = (unsigned char)v; }
  return d;
}

static std::vector<float> readPoints(std::istream &in, int rows) {
  std::vector<float> p(2 * (size_t)rows);
  for (auto &v : p) in >> v;
  return p;
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  int desc_bytes, n_hyp, n_rec, n_cur, ncm, ncs, nrm, nrs;
  double min_distance, ratio, fx, fy, cx, cy, threshold;
  unsigned long seed;
  in >> desc_bytes >> min_distance >> ratio >> fx >> fy >> cx >> cy >> threshold >> n_hyp >> seed;
  in >> n_rec >> n_cur >> ncm >> ncs >> nrm >> nrs;
  if (!in) { std::fprintf(stderr, "bad case file\n"); return 2; }
  const Descriptors rec = readDesc(in, n_rec, desc_bytes);
  const std::vector<float> rec_px = readPoints(in, n_rec);
  const Descriptors cur = readDesc(in, n_cur, desc_bytes);
  const std::vector<float> cur_px = readPoints(in, n_cur);
  // the matching half needs no vocabulary: the smallest tree xk_pr_create accepts
  PRVocabulary v;
  v.k = 1; v.L = 1; v.kmax = 1; v.desc_bytes = desc_bytes;
  v.node_desc.assign(2 * (size_t)desc_bytes, 0);
  v.children = {1, -1};
  v.word_of_node = {-1, 0};
  v.node_of_word = {1};
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  try {
    Database db(xk, v, 0.6, 0, 0, 1024);
    std::vector<int> idx, dist;
    db.knnMatch(rec, cur, idx, dist);                                               // :249
    std::printf("K");
    for (int q = 0; q < n_rec; ++q) std::printf(" %d:%d:%d:%d", idx[2 * q], dist[2 * q], idx[2 * q + 1], dist[2 * q + 1]);
    std::printf("\n");
    const std::vector<GoodMatch> good = goodMatches(idx, dist, min_distance, ratio);   // :252-263
    std::printf("G");
    for (const GoodMatch &g : good) std::printf(" %d:%d", g.queryIdx, g.trainIdx);
    std::printf("\n");
    // :264-267 -- the points of the ratio-test survivors, before duplicate removal (which the mask precedes)
    const std::vector<GoodMatch> cand = ratioTestMatches(idx, dist, min_distance, ratio);
    std::vector<float> cp, rp;
    for (const GoodMatch &g : cand) {
      cp.push_back(cur_px[2 * g.trainIdx]); cp.push_back(cur_px[2 * g.trainIdx + 1]);
      rp.push_back(rec_px[2 * g.queryIdx]); rp.push_back(rec_px[2 * g.queryIdx + 1]);
    }
    const std::vector<unsigned char> mask = db.essentialInliers(cp, rp, fx, fy, cx, cy, threshold, n_hyp, seed);   // :269-274
    int n_inl = 0;
    for (unsigned char m : mask) n_inl += m;
    std::printf("E %d ", n_inl);
    for (unsigned char m : mask) std::printf("%d", (int)m);
    std::printf("\n");
    const std::vector<GoodMatch> filtered = goodMatches(idx, dist, min_distance, ratio, &mask);   // :275-301
    std::printf("F");
    for (const GoodMatch &g : filtered) std::printf(" %d:%d", g.queryIdx, g.trainIdx);
    std::printf("\n");
    std::printf("C");
    for (const ClassifiedMatch &c : classifyMatches(filtered, ncm, ncs, nrm, nrs)) std::printf(" %d:%d:%d", (int)c.kind, c.current, c.received);
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    xk_destroy(xk);
    return 1;
  }
  xk_destroy(xk);
  return 0;
}
