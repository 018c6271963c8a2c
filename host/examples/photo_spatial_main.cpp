// The spatial photometric map on the mirror (x::FeatureTracker::setSpatialCalibration): synthetic frames of one
// texture seen through a known smooth map (a radial fall-off), the view moving a few pixels per frame; every frame after the first
// goes through calibrate() until the coverage passes the threshold and the estimate installs its map.  Nothing is read from disk:
// the texture comes from a fixed linear congruential sequence.
//   usage  : xk_photo_spatial_example [max_frames] [div] [coverage threshold]
//   output : F <frame> <kept> <rows> <covered>/<cells>        per calibrated frame
//            S <rows> <covered> <cells> <ready> <dropped> <state>   the status after the last frame
//            O <n> <ls iterations> <gp iterations> <ls residual> <gp residual> <converged>
//            M <rms of the true map about its mean> <rms of (estimate - true) about its mean> <calibrated>
// The map is determined up to a constant (the gauge of the least squares), so both figures of M are taken about the mean.
// A row states the map's difference over a feature's displacement (here <= 5 pixels) as the difference of two cells whose centres
// lie div = 16 pixels apart, so the model of irPhotoCalib.cpp:162-198 recovers the map's shape at a fraction of its amplitude (the
// NumPy restatement gives 0.12 of it from noise-free rows of 5-pixel displacements, 0.37 at 16): the second figure of M is expected
// a little below the first, not near zero.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "x/vision/feature_tracker.h"

using namespace x;

static const int W = 160, H = 128, PAD = 48, KERNEL = 8;

static double true_map(int x, int y) {
  const double u = (x - 0.5 * (W - 1)) / (0.5 * W), v = (y - 0.5 * (H - 1)) / (0.5 * H);
  return -0.03 * (u * u + v * v);
}

// Tracker::computeIntensity of the caller's own frame: the box mean around (x, y), as the device takes it
static double box_mean(const std::vector<uint8_t> &img, int x, int y) {
  const int hk = KERNEL / 2;
  long sum = 0, cnt = 0;
  for (int r = std::max(y - hk, 0); r < std::min(y + hk, H); ++r)
    for (int c = std::max(x - hk, 0); c < std::min(x + hk, W); ++c) { sum += img[(size_t)r * W + c]; ++cnt; }
  return cnt > 0 ? (double)sum / (255.0 * (double)cnt) : 0.0;
}

int main(int argc, char **argv) {
  const int max_frames = argc > 1 ? std::atoi(argv[1]) : 120, div = argc > 2 ? std::atoi(argv[2]) : 16;
  // 0.97 rather than the reference's 0.9, which three frames that all move one way already reach: a few frames more put rows of
  // more than one direction into the estimate
  const double thr = argc > 3 ? std::atof(argv[3]) : 0.97;
  // the texture: blocks of 4 x 4 pixels of a seeded grey, on a canvas larger than the view by PAD on every side
  const int CW = W + 2 * PAD, CH = H + 2 * PAD;
  std::vector<uint8_t> canvas((size_t)CW * CH);
  unsigned int lcg = 12345u;
  std::vector<uint8_t> blocks((size_t)(CW / 4 + 1) * (CH / 4 + 1));
  for (uint8_t &b : blocks) { lcg = lcg * 1664525u + 1013904223u; b = (uint8_t)(60 + (lcg >> 24) % 120); }
  for (int y = 0; y < CH; ++y)
    for (int x = 0; x < CW; ++x) canvas[(size_t)y * CW + x] = blocks[(size_t)(y / 4) * (CW / 4 + 1) + x / 4];
  const auto offset = [](int f, int &ox, int &oy) {             // a closed path around the canvas' centre, <= 5 pixels per frame
    const double t = 2.0 * 3.14159265358979323846 * f / 40.0;
    ox = PAD + (int)std::lround(30.0 * std::sin(t)); oy = PAD + (int)std::lround(12.0 * std::sin(2.0 * t));
  };
  const auto render = [&](int f) {
    int ox, oy;
    offset(f, ox, oy);
    std::vector<uint8_t> img((size_t)W * H);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const double v = canvas[(size_t)(y + oy) * CW + x + ox] + 255.0 * true_map(x, y);
        img[(size_t)y * W + x] = (uint8_t)std::min(255.0, std::max(0.0, std::floor(v + 0.5)));
      }
    return img;
  };
  const Camera camera(1.0, 1.0, 0.5, 0.5, 0.0, W, H);            // (the calibration never reads the intrinsics)
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    FeatureTracker tracker(xk, camera, 2048, 11, 11, 2, 30, 0.01, 1e-4);
    tracker.setDetection(12, true, 3, 8);
    tracker.setPhotometric(KERNEL, 0.0, 0.0, 256);
    tracker.setSpatialCalibration(div, thr);
    // the features: the corners detected in four views a quarter of the path apart, kept in canvas coordinates.  The view's motion is
    // known, so every frame's previous list is these corners where they lie in the previous view, with their box means there
    std::vector<std::pair<int, int>> corners;
    for (int f : {0, 10, 20, 30}) {
      int ox, oy;
      offset(f, ox, oy);
      const std::vector<uint8_t> img = render(f);
      tracker.pushImage(img.data(), W);
      for (const TrackedFeature &p : tracker.detect(FeatureList())) corners.emplace_back((int)p.getXDist() + ox, (int)p.getYDist() + oy);
    }
    std::vector<uint8_t> prev = render(0);
    tracker.pushImage(prev.data(), W);
    int frame = 1;
    for (; frame < max_frames && !tracker.spatialCalibrated(); ++frame) {
      int pox, poy;
      offset(frame - 1, pox, poy);
      FeatureList previous;
      for (const auto &c : corners) {
        const int x = c.first - pox, y = c.second - poy;
        if (x < 8 || y < 8 || x >= W - 8 || y >= H - 8 || (int)previous.size() >= 2048) continue;
        // at the pixel's centre: the view moves by whole pixels, so the tracked position stays half a pixel away from where the
        // truncation to a pixel (tracker.cpp:807-808) would flip
        TrackedFeature p(x + 0.5, y + 0.5, x + 0.5, y + 0.5);
        p.setIntensity(box_mean(prev, x, y));
        previous.push_back(p);
      }
      const std::vector<uint8_t> cur = render(frame);
      tracker.pushImage(cur.data(), W);
      const FeatureTracker::Calibration c = tracker.calibrate(previous, (unsigned long)frame);
      const FeatureTracker::SpatialStatus s = tracker.spatialStatus();
      std::printf("F %d %d %d %d/%d\n", frame, c.kept, s.rows, s.covered, s.cells);
      prev = cur;
    }
    const FeatureTracker::SpatialStatus s = tracker.spatialStatus();
    std::printf("S %d %d %d %d %d %d\n", s.rows, s.covered, s.cells, s.ready ? 1 : 0, s.dropped, s.state);
    const xk_photo_spatial_outcome &o = tracker.spatialOutcome();
    std::printf("O %d %d %d %.3g %.3g %d\n", o.n, o.ls_iterations, o.gp_iterations, o.ls_residual, o.gp_residual, o.converged);
    double rms_true = 0.0, rms_err = 0.0;
    if (tracker.spatialCalibrated()) {
      const std::vector<float> ps = tracker.spatialMap();
      double mt = 0.0, me = 0.0;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) { mt += true_map(x, y); me += ps[(size_t)y * W + x] - true_map(x, y); }
      mt /= (double)W * H; me /= (double)W * H;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const double t = true_map(x, y) - mt, e = ps[(size_t)y * W + x] - true_map(x, y) - me;
          rms_true += t * t; rms_err += e * e;
        }
      rms_true = std::sqrt(rms_true / ((double)W * H)); rms_err = std::sqrt(rms_err / ((double)W * H));
    }
    std::printf("M %.6g %.6g %d\n", rms_true, rms_err, tracker.spatialCalibrated() ? 1 : 0);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
