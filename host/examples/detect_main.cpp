// The front end of Tracker::track (tracker.cpp:131-310) on the mirror, from images to the frame's matches: detection on the first
// image; on every later one tracking, removeOverflowFeatures, re-detection around the survivors when fewer than n_feat_min are
// left -- on the previous image, the reference's stated arguments (:214) -- tracking of the new ones, concatenation and the
// outlier removal.  Raw images from files (written by tests/test_gpu_fast_host.py), one printed line per list.
//   usage  : xk_detect_example case.txt image1.raw image2.raw ...
//   case   : fx fy cx cy s width height stride win_w win_h max_level max_iter eps min_eig_thr threshold_px n_hyp seed max_features
//            fast_threshold non_max_supp block_half_length margin max_candidates n_tiles_h n_tiles_w max_feat_per_tile n_feat_min
//            (fx ... cy as fractions of the image size; the raw files hold height rows of stride bytes)
//   output : D f n  x y score ...                    frame f: detected on the first image
//            T f n  px py cx cy ...                  pairs the tracking kept (distorted pixels, %.17g)
//            O f n  px py cx cy prow pcol crow ccol ...   after removeOverflow, with the tiles
//            R f n  x y score ...                    re-detected on the previous image
//            A f n  px py cx cy ...                  after the new pairs were appended
//            M f n  pxd pyd cxd cyd px py cx cy ...  the matches: distorted, then undistorted pixels
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

static void print_detected(const char *tag, int frame, const FeatureList &l) {
  std::printf("%s %d %zu", tag, frame, l.size());
  for (const TrackedFeature &f : l) std::printf(" %.17g %.17g %.17g", f.getXDist(), f.getYDist(), f.getFastScore());
  std::printf("\n");
}

static void print_pairs(const char *tag, int frame, const FeatureList &a, const FeatureList &b, bool tiles) {
  std::printf("%s %d %zu", tag, frame, a.size());
  for (size_t i = 0; i < a.size(); ++i) {
    std::printf(" %.17g %.17g %.17g %.17g", a[i].getXDist(), a[i].getYDist(), b[i].getXDist(), b[i].getYDist());
    if (tiles) std::printf(" %d %d %d %d", a[i].getTileRow(), a[i].getTileCol(), b[i].getTileRow(), b[i].getTileCol());
  }
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s case.txt image1.raw image2.raw ...\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, eps, min_eig_thr, threshold;
  unsigned int width, height, n_tiles_h, n_tiles_w, max_feat_per_tile, n_feat_min;
  int stride, win_w, win_h, max_level, max_iter, n_hyp, max_features, fast_threshold, non_max_supp, block_half_length, margin, max_candidates;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> stride >> win_w >> win_h >> max_level >> max_iter >> eps >> min_eig_thr >> threshold >>
      n_hyp >> seed >> max_features >> fast_threshold >> non_max_supp >> block_half_length >> margin >> max_candidates >> n_tiles_h >>
      n_tiles_w >> max_feat_per_tile >> n_feat_min;
  if (!in || stride < (int)width) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<std::vector<uint8_t>> images((size_t)argc - 2);
  for (int i = 2; i < argc; ++i)
    if (!read_raw(argv[i], (size_t)stride * height, images[(size_t)i - 2])) { std::fprintf(stderr, "bad image file %s\n", argv[i]); return 2; }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    FeatureTracker tracker(xk, camera, max_features, win_w, win_h, max_level, max_iter, eps, min_eig_thr);
    tracker.setDetection(fast_threshold, non_max_supp != 0, block_half_length, margin, max_candidates);
    MatchFilter filter(xk, camera, max_features, threshold, n_hyp, seed);
    TileGrid grid(width, height, n_tiles_h, n_tiles_w, max_feat_per_tile);
    FeatureList previous_features;
    for (size_t f = 0; f < images.size(); ++f) {
      const int frame = (int)f + 1;
      tracker.pushImage(images[f].data(), stride);
      FeatureList current_features;
      if (frame == 1) {                                          // tracker.cpp:160-167
        current_features = tracker.detect(FeatureList());
        print_detected("D", frame, current_features);
      } else {
        std::pair<FeatureList, FeatureList> pairs = tracker.track(previous_features);             // :193-195
        previous_features = std::move(pairs.first);
        current_features = std::move(pairs.second);
        print_pairs("T", frame, previous_features, current_features, false);
        FeatureTracker::removeOverflow(grid, previous_features, current_features);               // :200-201
        print_pairs("O", frame, previous_features, current_features, true);
        if (current_features.size() < n_feat_min) {                                               // :204-228
          const FeatureList previous_new = tracker.detect(previous_features, false);
          print_detected("R", frame, previous_new);
          std::pair<FeatureList, FeatureList> fresh = tracker.track(previous_new);
          previous_features.insert(previous_features.end(), fresh.first.begin(), fresh.first.end());
          current_features.insert(current_features.end(), fresh.second.begin(), fresh.second.end());
          print_pairs("A", frame, previous_features, current_features, false);
        }
        const MatchList matches = filter.filter(previous_features, current_features);             // :233-293
        std::printf("M %d %zu", frame, matches.size());
        current_features.clear();
        for (const Match &m : matches) {
          std::printf(" %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", m.previous.getXDist(), m.previous.getYDist(), m.current.getXDist(),
                      m.current.getYDist(), m.previous.getX(), m.previous.getY(), m.current.getX(), m.current.getY());
          current_features.push_back(m.current);
        }
        std::printf("\n");
      }
      previous_features = current_features;                      // :299
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
