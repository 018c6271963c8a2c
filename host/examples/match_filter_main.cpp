// The outlier removal of Tracker::track (tracker.cpp:233-293) on the mirror, from a text case file (written by
// tests/test_gpu_match_filter_host.py), one printed line per result.
//   header : fx fy cx cy s width height threshold n_hyp seed max_matches      (fx ... cy as fractions of the image size)
//   size   : n
//   rows   : previous x_dist y_dist, current x_dist y_dist
//   output : N <kept>                                    number of matches
//            I <index ...>                               positions of the kept pairs
//            M <px py cx cy ...>                         undistorted pixels of the kept pairs, %.17g
//            U <x y>                                     Camera::undistort of the first previous feature on the host
#include <cstdio>
#include <fstream>
#include <iostream>

#include "x/vision/match_filter.h"

using namespace x;

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, threshold;
  unsigned int width, height;
  int n_hyp, max_matches, n;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> threshold >> n_hyp >> seed >> max_matches >> n;
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
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  try {
    MatchFilter filter(xk, camera, max_matches, threshold, n_hyp, seed);
    std::vector<int> kept;
    const MatchList matches = filter.filter(previous, current, &kept);
    std::printf("N %zu\nI", matches.size());
    for (int k : kept) std::printf(" %d", k);
    std::printf("\nM");
    for (const Match &m : matches)
      std::printf(" %.17g %.17g %.17g %.17g", m.previous.getX(), m.previous.getY(), m.current.getX(), m.current.getY());
    std::printf("\n");
    if (n > 0) {
      TrackedFeature f = previous[0];
      camera.undistort(f);
      std::printf("U %.17g %.17g\n", f.getX(), f.getY());
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    xk_destroy(xk);
    return 1;
  }
  xk_destroy(xk);
  return 0;
}
