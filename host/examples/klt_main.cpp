// Tracker::featureTracking and the outlier removal behind it (tracker.cpp:623-690, :233-293) on the mirror: two raw images and a
// point list from files (written by tests/test_gpu_klt_host.py), tracked by x::FeatureTracker, the kept pairs filtered by
// x::MatchFilter, one printed line per result.
//   usage  : xk_klt_example case.txt previous.raw current.raw points.txt
//   case   : fx fy cx cy s width height stride win_w win_h max_level max_iter eps min_eig_thr threshold n_hyp seed max_features
//            (fx ... cy as fractions of the image size; the raw files hold height rows of stride bytes)
//   points : n, then n rows x_dist y_dist
//   output : T <tracked>                                 pairs the tracking kept
//            J <index ...>                               their positions in the point list
//            C <x y ...>                                 where they are in the current image, %.17g
//            N <kept>                                    matches the filter kept
//            I <index ...>                               their positions among the tracked pairs
//            M <px py cx cy ...>                         undistorted pixels of the matches, %.17g
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>

#include "x/vision/feature_tracker.h"
#include "x/vision/match_filter.h"

using namespace x;

static bool read_raw(const char *path, size_t bytes, std::vector<uint8_t> &out) {
  std::ifstream f(path, std::ios::binary);
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return out.size() == bytes;
}

int main(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s case.txt previous.raw current.raw points.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, eps, min_eig_thr, threshold;
  unsigned int width, height;
  int stride, win_w, win_h, max_level, max_iter, n_hyp, max_features, n;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> stride >> win_w >> win_h >> max_level >> max_iter >> eps >> min_eig_thr >> threshold >>
      n_hyp >> seed >> max_features;
  if (!in || stride < (int)width) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<uint8_t> previous_img, current_img;
  if (!read_raw(argv[2], (size_t)stride * height, previous_img) || !read_raw(argv[3], (size_t)stride * height, current_img)) {
    std::fprintf(stderr, "bad image file\n");
    return 2;
  }
  std::ifstream pin(argv[4]);
  pin >> n;
  if (!pin || n < 0) { std::fprintf(stderr, "bad point file\n"); return 2; }
  FeatureList previous;
  for (int i = 0; i < n; ++i) {
    double a, b;
    pin >> a >> b;
    previous.emplace_back(0.0, 0.0, a, b);
  }
  if (!pin) { std::fprintf(stderr, "bad point file\n"); return 2; }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    FeatureTracker tracker(xk, camera, max_features, win_w, win_h, max_level, max_iter, eps, min_eig_thr);
    MatchFilter filter(xk, camera, max_features, threshold, n_hyp, seed);
    tracker.pushImage(previous_img.data(), stride);
    tracker.pushImage(current_img.data(), stride);
    std::vector<int> tracked, kept;
    const std::pair<FeatureList, FeatureList> pairs = tracker.track(previous, &tracked);
    std::printf("T %zu\nJ", pairs.first.size());
    for (int k : tracked) std::printf(" %d", k);
    std::printf("\nC");
    for (const TrackedFeature &f : pairs.second) std::printf(" %.17g %.17g", f.getXDist(), f.getYDist());
    const MatchList matches = filter.filter(pairs.first, pairs.second, &kept);
    std::printf("\nN %zu\nI", matches.size());
    for (int k : kept) std::printf(" %d", k);
    std::printf("\nM");
    for (const Match &m : matches)
      std::printf(" %.17g %.17g %.17g %.17g", m.previous.getX(), m.previous.getY(), m.current.getX(), m.current.getY());
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
