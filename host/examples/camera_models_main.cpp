// x::Camera::setDistortion on the mirror -- the radial-tangential and the equidistant lens of xk_trk_camera_model --
// beside the device: the host camera's undistortion of a frame's pairs, the device's (xk_trk_undistort), and x::MatchFilter::filter of
// the same pairs.  From a text case file (written by tests/test_gpu_camera_models_host.py), one printed line per result.
//   header : fx fy cx cy width height threshold n_hyp seed max_matches        (fx ... cy as fractions of the image size)
//   model  : model n_coeffs coeff ...
//   size   : n
//   rows   : previous x_dist y_dist, current x_dist y_dist
//   output : H <x y ...>                                 Camera::undistort of the previous, then the current features, %.17g
//            V <0|1 ...>                                 1: that point is valid on the host
//            D <x y ...>                                 xk_trk_undistort of the same 2n points
//            S <n_invalid> <max_steps>                   xk_trk_undistort_status after it
//            R <u v>                                     Camera::distort of the first H point
//            N <kept>                                    number of matches of MatchFilter::filter
//            I <index ...>                               positions of the kept pairs
//            M <px py cx cy ...>                         undistorted pixels of the kept pairs
#include <cstdio>
#include <fstream>
#include <initializer_list>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "x/vision/match_filter.h"

using namespace x;

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, threshold;
  unsigned int width, height;
  int n_hyp, max_matches, n, model, n_coeffs;
  unsigned long seed;
  in >> fx >> fy >> cx >> cy >> width >> height >> threshold >> n_hyp >> seed >> max_matches >> model >> n_coeffs;
  if (!in || n_coeffs < 0 || n_coeffs > 5) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<double> coeffs((size_t)n_coeffs);
  for (double &c : coeffs) in >> c;
  in >> n;
  if (!in || n < 0 || 2 * n > max_matches) { std::fprintf(stderr, "bad case file\n"); return 2; }
  FeatureList previous, current;
  for (int i = 0; i < n; ++i) {
    double a, b, c, d;
    in >> a >> b >> c >> d;
    previous.emplace_back(0.0, 0.0, a, b);
    current.emplace_back(0.0, 0.0, c, d);
  }
  if (!in) { std::fprintf(stderr, "bad case file\n"); return 2; }
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  xk_trk *trk = nullptr;
  int rc = 0;
  try {
    Camera camera(fx, fy, cx, cy, 0.0, width, height);
    camera.setDistortion(model, coeffs);
    // the host camera
    std::vector<double> dist;
    for (const FeatureList *list : {&previous, &current})
      for (const TrackedFeature &f : *list) { dist.push_back(f.getXDist()); dist.push_back(f.getYDist()); }
    std::vector<double> host(dist.size()), dev(dist.size());
    std::vector<int> valid((size_t)(2 * n));
    for (int i = 0; i < 2 * n; ++i) valid[(size_t)i] = camera.undistort(dist[2 * i], dist[2 * i + 1], &host[2 * i], &host[2 * i + 1]) ? 1 : 0;
    std::printf("H");
    for (double v : host) std::printf(" %.17g", v);
    std::printf("\nV");
    for (int v : valid) std::printf(" %d", v);
    // the device, through the C ABI
    int n_invalid = -1, max_steps = -1;
    if (xk_trk_create(xk, max_matches, camera.getFx(), camera.getFy(), camera.getCx(), camera.getCy(), 0.0, &trk) != XK_OK ||
        xk_trk_camera_model(trk, model, coeffs.data(), n_coeffs) != XK_OK ||
        xk_trk_undistort(trk, dist.data(), 2 * n, dev.data()) != XK_OK || xk_trk_undistort_status(trk, &n_invalid, &max_steps) != XK_OK)
      throw std::runtime_error(std::string("device undistortion: ") + xk_last_error(xk));
    std::printf("\nD");
    for (double v : dev) std::printf(" %.17g", v);
    std::printf("\nS %d %d\n", n_invalid, max_steps);
    if (n > 0) {
      double u, v;
      camera.distort(host[0], host[1], &u, &v);
      std::printf("R %.17g %.17g\n", u, v);
    }
    // the filter of the mirror: it takes the camera's lens at construction
    MatchFilter filter(xk, camera, max_matches, threshold, n_hyp, seed);
    std::vector<int> kept;
    const MatchList matches = filter.filter(previous, current, &kept);
    std::printf("N %zu\nI", matches.size());
    for (int k : kept) std::printf(" %d", k);
    std::printf("\nM");
    for (const Match &m : matches)
      std::printf(" %.17g %.17g %.17g %.17g", m.previous.getX(), m.previous.getY(), m.current.getX(), m.current.getY());
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_trk_destroy(trk);
  xk_destroy(xk);
  return rc;
}
