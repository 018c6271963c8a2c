// outlier_method on the mirror (Tracker's outlier_method_, tracker.h:256): x::MatchFilter and x::Tracker under cv::LMEDS (4), cv::RANSAC
// (8) or any other value, from text case files (written by tests/test_gpu_lmeds_host.py).
//   usage  : xk_lmeds_example filter case.txt
//            xk_lmeds_example track case.txt image0.raw image1.raw ...
//   filter : fx fy cx cy s width height threshold n_hyp seed max_matches outlier_method, then n, then n rows
//            previous x_dist y_dist, current x_dist y_dist       (fx ... cy as fractions of the image size)
//   output : N <kept>                                    number of matches
//            I <index ...>                               positions of the kept pairs
//            M <px py cx cy ...>                         undistorted pixels of the kept pairs, %.17g
//            L <ran LMedS> <median> <sigma>              the winner's median and scale, %.17g (zeros after RANSAC)
//   track  : the case line of xk_tracker_example without its last three fields, then outlier_method
//   output : F <frame> <tracked> <left> <redetected> <candidates> <accepted> <new tracked> <matches> <winner>
//            C <x y x_dist y_dist ...>                   the current features of the matches, %.17g
//            L <ran LMedS> <median> <sigma>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>

#include "x/vision/match_filter.h"
#include "x/vision/tracker.h"

using namespace x;

static int run_filter(xk_handle *xk, std::ifstream &in) {
  double fx, fy, cx, cy, s, threshold;
  unsigned int width, height;
  int n_hyp, max_matches, method, n;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> threshold >> n_hyp >> seed >> max_matches >> method >> n;
  if (!in || n < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
  FeatureList previous, current;
  for (int i = 0; i < n; ++i) {
    double a, b, c, d;
    in >> a >> b >> c >> d;
    previous.emplace_back(0.0, 0.0, a, b);
    current.emplace_back(0.0, 0.0, c, d);
  }
  if (!in) { std::fprintf(stderr, "bad case file\n"); return 2; }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  MatchFilter filter(xk, camera, max_matches, threshold, n_hyp, seed, method);
  std::vector<int> kept;
  const MatchList matches = filter.filter(previous, current, &kept);
  std::printf("N %zu\nI", matches.size());
  for (int k : kept) std::printf(" %d", k);
  std::printf("\nM");
  for (const Match &m : matches)
    std::printf(" %.17g %.17g %.17g %.17g", m.previous.getX(), m.previous.getY(), m.current.getX(), m.current.getY());
  double median = 0.0, sigma = 0.0;
  const bool lmeds = filter.lastLmeds(&median, &sigma);
  std::printf("\nL %d %.17g %.17g\n", lmeds ? 1 : 0, median, sigma);
  return 0;
}

static int run_track(xk_handle *xk, std::ifstream &in, int n_img, char **img_path) {
  double fx, fy, cx, cy, s, min_eig_thr, threshold_px;
  unsigned int width, height, block_half_length, margin, n_feat_min, n_tiles_h, n_tiles_w, max_feat_per_tile;
  int stride, win_w, win_h, max_level, fast_threshold, non_max_supp, n_hyp, max_features, method;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> stride >> win_w >> win_h >> max_level >> min_eig_thr >> fast_threshold >> non_max_supp >>
      block_half_length >> margin >> n_feat_min >> n_tiles_h >> n_tiles_w >> max_feat_per_tile >> threshold_px >> n_hyp >> seed >> max_features >>
      method;
  if (!in || stride < (int)width) { std::fprintf(stderr, "bad case file\n"); return 2; }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  Tracker tracker(xk, camera, fast_threshold, non_max_supp != 0, block_half_length, margin, n_feat_min, method, threshold_px, 0.99, win_w, win_h,
                  max_level, min_eig_thr, max_features, n_hyp);
  tracker.setTiles(n_tiles_h, n_tiles_w, max_feat_per_tile);
  tracker.setSeed(seed);
  std::vector<uint8_t> img;
  for (int i = 0; i < n_img; ++i) {
    std::ifstream f(img_path[i], std::ios::binary);
    img.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    if (img.size() != (size_t)stride * height) { std::fprintf(stderr, "bad image file %s\n", img_path[i]); return 2; }
    const MatchList &matches = tracker.track(img.data(), stride, 0.1 * i, (unsigned int)i);
    const xk_trk_frame_out &c = tracker.counts();
    std::printf("F %d %d %d %d %d %d %d %d %d\nC", i, c.n_tracked, c.n_left, c.redetected, c.n_candidates, c.n_accepted, c.n_new_tracked,
                c.n_matches, c.winner);
    for (const Match &m : matches) std::printf(" %.17g %.17g %.17g %.17g", m.current.getX(), m.current.getY(), m.current.getXDist(), m.current.getYDist());
    double median = 0.0, sigma = 0.0;
    const bool lmeds = tracker.lastLmeds(&median, &sigma);
    std::printf("\nL %d %.17g %.17g\n", lmeds ? 1 : 0, median, sigma);
  }
  return 0;
}

int main(int argc, char **argv) {
  const bool filter = argc == 3 && !std::strcmp(argv[1], "filter"), track = argc >= 4 && !std::strcmp(argv[1], "track");
  if (!filter && !track) { std::fprintf(stderr, "usage: %s filter case.txt | track case.txt image0.raw ...\n", argv[0]); return 2; }
  std::ifstream in(argv[2]);
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc;
  try {
    rc = filter ? run_filter(xk, in) : run_track(xk, in, argc - 3, argv + 3);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
