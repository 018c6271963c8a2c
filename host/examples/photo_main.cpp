// Tracker::calibrateImage in front of Tracker::featureTracking (tracker.cpp:186-195, :761-858) on the mirror: two raw images from
// files (written by tests/test_gpu_photo_host.py), the first one's features detected by x::FeatureTracker, the second calibrated
// against them and then tracked, one printed line per result.
//   usage  : xk_photo_example case.txt previous.raw current.raw
//   case   : width height stride win_w win_h max_level max_iter eps min_eig_thr threshold block_half_length margin kernel_size
//            epsilon_gap epsilon_base n_hyp seed max_features   (the raw files hold height rows of stride bytes)
//   output : D <detected>                                features of the first image
//            P <x y intensity ...>                       their pixels and intensities, %.17g
//            E <estimated> <kept> <support>              of the calibration
//            G <a_rel b_rel w_a w_b a b>                 the estimate, the adjusted pair, the frame's origin pair, %.17g
//            S <fnv-1a 64 of the corrected image> <of the raw image>
//            T <tracked>                                 pairs the tracking kept on the corrected image
//            J <index ...>                               their positions in the detected list
//            C <x y intensity ...>                       where they are in the current image and their raw intensities, %.17g
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>

#include "x/vision/feature_tracker.h"

using namespace x;

static bool read_raw(const char *path, size_t bytes, std::vector<uint8_t> &out) {
  std::ifstream f(path, std::ios::binary);
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return out.size() == bytes;
}

static unsigned long long fnv1a(const std::vector<uint8_t> &v) {
  unsigned long long h = 0xcbf29ce484222325ull;
  for (uint8_t b : v) { h ^= b; h *= 0x100000001b3ull; }
  return h;
}

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s case.txt previous.raw current.raw\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double eps, min_eig_thr, epsilon_gap, epsilon_base;
  unsigned int width, height;
  int stride, win_w, win_h, max_level, max_iter, threshold, b, margin, kernel_size, n_hyp, max_features;
  unsigned long seed;
  in >> width >> height >> stride >> win_w >> win_h >> max_level >> max_iter >> eps >> min_eig_thr >> threshold >> b >> margin >> kernel_size >>
      epsilon_gap >> epsilon_base >> n_hyp >> seed >> max_features;
  if (!in || stride < (int)width) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<uint8_t> previous_img, current_img;
  if (!read_raw(argv[2], (size_t)stride * height, previous_img) || !read_raw(argv[3], (size_t)stride * height, current_img)) {
    std::fprintf(stderr, "bad image file\n");
    return 2;
  }
  const Camera camera(1.0, 1.0, 0.5, 0.5, 0.0, width, height);   // (the calibration and the tracking never read the intrinsics)
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    FeatureTracker tracker(xk, camera, max_features, win_w, win_h, max_level, max_iter, eps, min_eig_thr);
    tracker.setDetection(threshold, true, b, margin);
    tracker.setPhotometric(kernel_size, epsilon_gap, epsilon_base, n_hyp);
    tracker.pushImage(previous_img.data(), stride);
    const FeatureList previous = tracker.detect(FeatureList());    // (the first frame is not calibrated: raw = working)
    std::printf("D %zu\nP", previous.size());
    for (const TrackedFeature &f : previous) std::printf(" %.17g %.17g %.17g", f.getXDist(), f.getYDist(), f.getIntensity());
    tracker.pushImage(current_img.data(), stride);
    const FeatureTracker::Calibration c = tracker.calibrate(previous, seed);
    std::printf("\nE %d %d %d\n", c.estimated ? 1 : 0, c.kept, c.support);
    std::printf("G %.17g %.17g %.17g %.17g %.17g %.17g\n", c.a_rel, c.b_rel, c.frame_ab[0], c.frame_ab[1], c.frame_ab[2], c.frame_ab[3]);
    std::printf("S %llu %llu\n", fnv1a(tracker.image(true, false)), fnv1a(tracker.image(true, true)));
    std::vector<int> tracked;
    const std::pair<FeatureList, FeatureList> pairs = tracker.track(previous, &tracked);
    std::printf("T %zu\nJ", pairs.first.size());
    for (int k : tracked) std::printf(" %d", k);
    std::printf("\nC");
    for (const TrackedFeature &f : pairs.second) std::printf(" %.17g %.17g %.17g", f.getXDist(), f.getYDist(), f.getIntensity());
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
