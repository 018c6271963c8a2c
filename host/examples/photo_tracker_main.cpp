// Tracker::track of a PHOTOMETRIC_CALI build (tracker.cpp:134-306 with calibrateImage at :186-190) on the mirror: a case file and raw
// images from files (written by tests/test_gpu_photo_frame_host.py), every image through the photometric x::Tracker, one block of
// lines per frame.
//   usage  : xk_photo_tracker_example [--second win_w win_h max_level min_eig_thr] case.txt image0.raw image1.raw ...
//            --second: the second Lucas-Kanade parameter set (Tracker::setSecondKlt), which the frames switch to once the
//            calibration is done
//   case   : fx fy cx cy s width height stride win_w win_h max_level min_eig_thr fast_threshold non_max_supp block_half_length margin
//            n_feat_min n_tiles_h n_tiles_w max_feat_per_tile threshold_px n_hyp seed max_features describe centroid edge
//            kernel_size epsilon_gap epsilon_base n_hyp_photo fast_threshold_photo seed_photo
//            (fx ... cy as fractions of the image size; the raw files hold height rows of stride bytes; frame i draws with seed + i
//            and seed_photo + i)
//   output : F <frame> <tracked> <left> <redetected> <candidates> <accepted> <new tracked> <matches> <winner>
//            G <kept> <estimated> <done> <support> <a_rel> <b_rel> <frame_ab x 4>     the frame's calibration, %.17g
//            O <origin ...>                              where each match's feature was in the previous frame's match list
//            I <previous current ...>                    getIntensity() of both features of each match, %.17g
//            K <set>                                     with --second only: the set the frame's feature trackings ran with
//            X <checksum>                                FNV-1a (64 bits, hex) over the bytes of every match in order: the previous
//                                                        feature's x y x_dist y_dist, the current one's, both intensities (fp64), the
//                                                        FAST score, the four tile indices (int32) and the descriptor
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Fnv {
  unsigned long long h = 0xcbf29ce484222325ull;
  void bytes(const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  }
  void f64(double v) { bytes(&v, sizeof v); }
  void i32(int v) { bytes(&v, sizeof v); }
};

int main(int argc, char **argv) {
  bool second = false;
  int win_w2 = 0, win_h2 = 0, max_level2 = 0;
  double min_eig_thr2 = 0.0;
  if (argc >= 6 && std::strcmp(argv[1], "--second") == 0) {
    second = true;
    win_w2 = std::atoi(argv[2]); win_h2 = std::atoi(argv[3]); max_level2 = std::atoi(argv[4]); min_eig_thr2 = std::atof(argv[5]);
    argc -= 5; argv += 5;
  }
  if (argc < 3) { std::fprintf(stderr, "usage: %s [--second win_w win_h max_level min_eig_thr] case.txt image0.raw image1.raw ...\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, min_eig_thr, threshold_px, eps_gap, eps_base;
  unsigned int width, height, block_half_length, margin, n_feat_min, n_tiles_h, n_tiles_w, max_feat_per_tile;
  int stride, win_w, win_h, max_level, fast_threshold, non_max_supp, n_hyp, max_features, describe, centroid, edge;
  int kernel_size, n_hyp_photo, fast_threshold_photo;
  unsigned long seed, seed_photo;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> stride >> win_w >> win_h >> max_level >> min_eig_thr >> fast_threshold >> non_max_supp >>
      block_half_length >> margin >> n_feat_min >> n_tiles_h >> n_tiles_w >> max_feat_per_tile >> threshold_px >> n_hyp >> seed >> max_features >>
      describe >> centroid >> edge >> kernel_size >> eps_gap >> eps_base >> n_hyp_photo >> fast_threshold_photo >> seed_photo;
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
    if (second) tracker.setSecondKlt(win_w2, win_h2, max_level2, min_eig_thr2);
    tracker.setPhotometric(kernel_size, eps_gap, eps_base, n_hyp_photo, fast_threshold_photo);
    tracker.setSeed(seed);
    tracker.setPhotoSeed(seed_photo);
    std::vector<uint8_t> img;
    for (int i = 2; i < argc; ++i) {
      if (!read_raw(argv[i], (size_t)stride * height, img)) { std::fprintf(stderr, "bad image file %s\n", argv[i]); rc = 2; break; }
      const MatchList &matches = tracker.track(img.data(), stride, 0.1 * (i - 2), (unsigned int)(i - 2));
      const xk_trk_frame_out &c = tracker.counts();
      const Tracker::Calibration &g = tracker.calibration();
      std::printf("F %d %d %d %d %d %d %d %d %d\n", i - 2, c.n_tracked, c.n_left, c.redetected, c.n_candidates, c.n_accepted, c.n_new_tracked,
                  c.n_matches, c.winner);
      std::printf("G %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\nO", g.kept, g.estimated ? 1 : 0, g.done ? 1 : 0, g.support, g.a_rel, g.b_rel,
                  g.frame_ab[0], g.frame_ab[1], g.frame_ab[2], g.frame_ab[3]);
      for (int o : tracker.origins()) std::printf(" %d", o);
      std::printf("\nI");
      Fnv sum;
      for (const Match &m : matches) {
        std::printf(" %.17g %.17g", m.previous.getIntensity(), m.current.getIntensity());
        for (const TrackedFeature *f : {&m.previous, &m.current}) { sum.f64(f->getX()); sum.f64(f->getY()); sum.f64(f->getXDist()); sum.f64(f->getYDist()); }
        sum.f64(m.previous.getIntensity()); sum.f64(m.current.getIntensity());
        sum.i32((int)m.current.getFastScore());
        sum.i32(m.previous.getTileRow()); sum.i32(m.previous.getTileCol()); sum.i32(m.current.getTileRow()); sum.i32(m.current.getTileCol());
        if (m.current.hasDescriptor()) sum.bytes(m.current.getDescriptor().data(), m.current.getDescriptor().size());
      }
      if (second) std::printf("\nK %d", tracker.lastKltSet());
      std::printf("\nX %016llx\n", sum.h);
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
