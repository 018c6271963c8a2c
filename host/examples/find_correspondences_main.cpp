// The non-GT branch of PlaceRecognition::findCorrespondences (place_recognition.cpp:137-385) as ONE call on the mirror,
// Database::findCorrespondences, from the text case file correspondences_main.cpp reads (written by
// tests/test_gpu_find_correspondences_host.py).
//   header : desc_bytes min_distance ratio fx fy cx cy threshold n_hyp seed
//   sizes  : n_rec n_cur n_cur_msckf n_cur_slam n_rec_msckf n_rec_slam
//   arrays : received descriptors, received pixels (x y per row), current descriptors, current pixels
//   output : S <status> <n_candidates> <n_inliers>
//            F <q:t ...>                                     the good matches: mask and duplicate removal applied
//            C <kind:current:received ...>                   their classification
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
    const Correspondences c = db.findCorrespondences(rec, rec_px, cur, cur_px, ncm, ncs, nrm, nrs, min_distance, ratio, fx, fy, cx,
                                                     cy, threshold, n_hyp, seed);
    std::printf("S %d %d %d\n", c.status, c.n_candidates, c.n_inliers);
    std::printf("F");
    for (const GoodMatch &g : c.good) std::printf(" %d:%d", g.queryIdx, g.trainIdx);
    std::printf("\n");
    std::printf("C");
    for (const ClassifiedMatch &m : c.classified) std::printf(" %d:%d:%d", (int)m.kind, m.current, m.received);
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    xk_destroy(xk);
    return 1;
  }
  xk_destroy(xk);
  return 0;
}
