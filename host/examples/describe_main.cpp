// Detection and description on the mirror, and the descriptors' way into the place recognition: two images, a scene and its copy
// shifted by a few pixels, go through x::FeatureTracker::detect with a description set up (PlaceRecognition::compute on the
// keypoints of a detection, tracker.cpp:440-444); the first image's features are tracked into the second, which hands their
// descriptors on (:675-679), and described again at the shifted pixels; x::Database::knnMatch (place_recognition.cpp:249) pairs
// those with the first image's.  Raw images from files (written by tests/test_gpu_orb_host.py), one printed line per list.
//   usage  : xk_describe_example case.txt vocabulary.txt image1.raw image2.raw
//   case   : fx fy cx cy s width height stride win_w win_h max_level max_iter eps min_eig_thr max_features
//            fast_threshold non_max_supp block_half_length margin max_candidates
//            centroid_orientation angle_deg edge max_descriptors shift_x shift_y n_pattern_rows (0 or 256) [x1 y1 x2 y2 ...]
//            (fx ... cy as fractions of the image size; the raw files hold height rows of stride bytes)
//   vocab  : k L n_nodes kmax desc_bytes n_words, then node_desc, children, word_of_node, node_of_word
//   output : D f n  x y score b0 ... b31 ...         image f: the detected features with their descriptors
//            T 2 n  px py cx cy b0 ... b31 ...       the pairs the tracking kept, with the CURRENT feature's descriptor
//            S 2 n  index b0 ... b31 ...             the raw block of the first image's features at the shifted pixels: their
//                                                    positions in the list and the rows
//            K 2 n  idx0 dist0 idx1 dist1 ...        the 2-NN of each row of S among the first image's descriptors
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>

#include "x/place_recognition/database.h"
#include "x/vision/feature_tracker.h"

using namespace x;

static bool read_raw(const char *path, size_t bytes, std::vector<uint8_t> &out) {
  std::ifstream f(path, std::ios::binary);
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return out.size() == bytes;
}

static void print_bytes(const unsigned char *b) {
  for (int i = 0; i < 32; ++i) std::printf(" %d", (int)b[i]);
}

static void print_detected(int frame, const FeatureList &l) {
  std::printf("D %d %zu", frame, l.size());
  for (const TrackedFeature &f : l) {
    std::printf(" %.17g %.17g %.17g", f.getXDist(), f.getYDist(), f.getFastScore());
    print_bytes(f.getDescriptor().data());
  }
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: %s case.txt vocabulary.txt image1.raw image2.raw\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, eps, min_eig_thr, angle_deg;
  unsigned int width, height;
  int stride, win_w, win_h, max_level, max_iter, max_features, fast_threshold, non_max_supp, block_half_length, margin, max_candidates;
  int centroid, edge, max_descriptors, shift_x, shift_y, n_pattern;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> stride >> win_w >> win_h >> max_level >> max_iter >> eps >> min_eig_thr >> max_features >>
      fast_threshold >> non_max_supp >> block_half_length >> margin >> max_candidates >> centroid >> angle_deg >> edge >> max_descriptors >>
      shift_x >> shift_y >> n_pattern;
  if (!in || stride < (int)width || (n_pattern != 0 && n_pattern != 256)) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<signed char> pattern((size_t)4 * n_pattern);
  for (auto &c : pattern) { int v; in >> v; c = (signed char)v; }
  std::ifstream vin(argv[2]);
  PRVocabulary voc;
  int nn, nw;
  vin >> voc.k >> voc.L >> nn >> voc.kmax >> voc.desc_bytes >> nw;
  if (!in || !vin || nn < 1 || nw < 1) { std::fprintf(stderr, "bad case or vocabulary file\n"); return 2; }
  voc.node_desc.resize((size_t)nn * voc.desc_bytes);
  for (auto &b : voc.node_desc) { int t; vin >> t; b = (unsigned char)t; }
  voc.children.resize((size_t)nn * voc.kmax);
  for (auto &c : voc.children) vin >> c;
  voc.word_of_node.resize((size_t)nn);
  for (auto &c : voc.word_of_node) vin >> c;
  voc.node_of_word.resize((size_t)nw);
  for (auto &c : voc.node_of_word) vin >> c;
  std::vector<uint8_t> images[2];
  for (int i = 0; i < 2; ++i)
    if (!read_raw(argv[3 + i], (size_t)stride * height, images[i])) { std::fprintf(stderr, "bad image file %s\n", argv[3 + i]); return 2; }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    FeatureTracker tracker(xk, camera, max_features, win_w, win_h, max_level, max_iter, eps, min_eig_thr);
    tracker.setDetection(fast_threshold, non_max_supp != 0, block_half_length, margin, max_candidates);
    tracker.setDescription(centroid != 0, angle_deg, edge, n_pattern ? pattern.data() : nullptr, max_descriptors);   // (raises the margin to edge)
    Database db(xk, voc, 0.0, 0, 0, max_descriptors);

    tracker.pushImage(images[0].data(), stride);
    const FeatureList first = tracker.detect(FeatureList());
    print_detected(1, first);

    tracker.pushImage(images[1].data(), stride);
    const std::pair<FeatureList, FeatureList> pairs = tracker.track(first);
    std::printf("T 2 %zu", pairs.first.size());
    for (size_t i = 0; i < pairs.first.size(); ++i) {
      std::printf(" %.17g %.17g %.17g %.17g", pairs.first[i].getXDist(), pairs.first[i].getYDist(), pairs.second[i].getXDist(),
                  pairs.second[i].getYDist());
      print_bytes(pairs.second[i].getDescriptor().data());
    }
    std::printf("\n");

    std::vector<std::pair<int, int>> moved;
    for (const TrackedFeature &f : first) moved.emplace_back((int)f.getXDist() + shift_x, (int)f.getYDist() + shift_y);
    std::vector<int> kept;
    const Descriptors second = tracker.describe(moved, true, &kept);
    std::printf("S 2 %d", second.rows);
    for (int i = 0; i < second.rows; ++i) {
      std::printf(" %d", kept[(size_t)i]);
      print_bytes(second.data.data() + 32 * (size_t)i);
    }
    std::printf("\n");
    print_detected(2, tracker.detect(FeatureList()));

    Descriptors train;
    train.rows = (int)first.size(); train.cols = 32;
    for (const TrackedFeature &f : first) train.data.insert(train.data.end(), f.getDescriptor().begin(), f.getDescriptor().end());
    std::vector<int> idx, dist;
    db.knnMatch(second, train, idx, dist);
    std::printf("K 2 %d", second.rows);
    for (int i = 0; i < second.rows; ++i) std::printf(" %d %d %d %d", idx[2 * (size_t)i], dist[2 * (size_t)i], idx[2 * (size_t)i + 1], dist[2 * (size_t)i + 1]);
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
