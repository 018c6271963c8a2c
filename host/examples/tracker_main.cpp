// Tracker::track (tracker.cpp:134-306) on the mirror: a case file and raw images from files (written by
// tests/test_gpu_tracker_frame_host.py), every image through x::Tracker::track, one block of lines per frame.
//   usage  : xk_tracker_example case.txt image0.raw image1.raw ...
//   case   : fx fy cx cy s width height stride win_w win_h max_level min_eig_thr fast_threshold non_max_supp block_half_length margin
//            n_feat_min n_tiles_h n_tiles_w max_feat_per_tile threshold_px n_hyp seed max_features describe centroid edge
//            (fx ... cy as fractions of the image size; the raw files hold height rows of stride bytes; frame i draws with seed + i)
//   output : F <frame> <tracked> <left> <redetected> <candidates> <accepted> <new tracked> <matches> <winner>
//            O <origin ...>                              where each match's feature was in the previous frame's match list
//            P <x y x_dist y_dist ...>                   the previous features of the matches, %.17g
//            C <x y x_dist y_dist ...>                   the current ones
//            S <score ...>                               FAST scores
//            T <row col row col ...>                     tiles of the previous and the current feature
//            D <hex ...>                                 descriptors, 64 hex digits each (with describe = 1)
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>

#include "x/vision/tracker.h"

using namespace x;

static bool read_raw(const char *path, size_t bytes, std::vector<uint8_t> &out) {
  std::ifstream f(path, std::ios::binary);
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return out.size() == bytes;
}

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s case.txt image0.raw image1.raw ...\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, min_eig_thr, threshold_px;
  unsigned int width, height, block_half_length, margin, n_feat_min, n_tiles_h, n_tiles_w, max_feat_per_tile;
  int stride, win_w, win_h, max_level, fast_threshold, non_max_supp, n_hyp, max_features, describe, centroid, edge;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> stride >> win_w >> win_h >> max_level >> min_eig_thr >> fast_threshold >> non_max_supp >>
      block_half_length >> margin >> n_feat_min >> n_tiles_h >> n_tiles_w >> max_feat_per_tile >> threshold_px >> n_hyp >> seed >> max_features >>
      describe >> centroid >> edge;
  if (!in || stride < (int)width) { std::fprintf(stderr, "bad case file\n"); return 2; }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    Tracker tracker(xk, camera, fast_threshold, non_max_supp != 0, block_half_length, margin, n_feat_min, 8, threshold_px, 0.99, win_w, win_h,
                    max_level, min_eig_thr, max_features, n_hyp);
    tracker.setTiles(n_tiles_h, n_tiles_w, max_feat_per_tile);
    if (describe) tracker.setDescription(centroid != 0, -1.0, edge);
    tracker.setSeed(seed);
    std::vector<uint8_t> img;
    for (int i = 2; i < argc; ++i) {
      if (!read_raw(argv[i], (size_t)stride * height, img)) { std::fprintf(stderr, "bad image file %s\n", argv[i]); rc = 2; break; }
      const MatchList &matches = tracker.track(img.data(), stride, 0.1 * (i - 2), (unsigned int)(i - 2));
      const xk_trk_frame_out &c = tracker.counts();
      std::printf("F %d %d %d %d %d %d %d %d %d\nO", i - 2, c.n_tracked, c.n_left, c.redetected, c.n_candidates, c.n_accepted, c.n_new_tracked,
                  c.n_matches, c.winner);
      for (int o : tracker.origins()) std::printf(" %d", o);
      std::printf("\nP");
      for (const Match &m : matches) std::printf(" %.17g %.17g %.17g %.17g", m.previous.getX(), m.previous.getY(), m.previous.getXDist(), m.previous.getYDist());
      std::printf("\nC");
      for (const Match &m : matches) std::printf(" %.17g %.17g %.17g %.17g", m.current.getX(), m.current.getY(), m.current.getXDist(), m.current.getYDist());
      std::printf("\nS");
      for (const Match &m : matches) std::printf(" %d", (int)m.current.getFastScore());
      std::printf("\nT");
      for (const Match &m : matches) std::printf(" %d %d %d %d", m.previous.getTileRow(), m.previous.getTileCol(), m.current.getTileRow(), m.current.getTileCol());
      std::printf("\nD");
      for (const Match &m : matches) {
        if (!m.current.hasDescriptor()) continue;
        std::printf(" ");
        for (unsigned char b : m.current.getDescriptor()) std::printf("%02x", b);
      }
      std::printf("\n");
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
