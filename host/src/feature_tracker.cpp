// Mirror of Tracker::featureTracking, src/x/vision/tracker.cpp:623-690; the arithmetic runs in libxk.so.
#include "x/vision/feature_tracker.h"

#include <stdexcept>
#include <string>

using namespace x;

static void check(xk_handle *h, int rc, const char *what) {
  if (rc != XK_OK) throw std::runtime_error(std::string(what) + ": " + xk_strerror(rc) + " (" + (h ? xk_last_error(h) : "") + ")");
}

FeatureTracker::FeatureTracker(xk_handle *xk, const Camera &camera, int max_features, int win_w, int win_h, int max_level, int max_iter,
                               double eps, double min_eig_thr)
    : xk_(xk) {
  if (max_features < 1) throw std::runtime_error("FeatureTracker: max_features < 1");
  const size_t m = (size_t)max_features;                      // (the staging first: nothing below can throw once the handle exists)
  prev_in_.resize(2 * m); cur_.resize(2 * m); min_eig_.resize(m); kept_prev_.resize(2 * m); kept_cur_.resize(2 * m);
  status_.resize(m); keep_.resize(m);
  check(xk_, xk_trk_create(xk_, max_features, camera.getFx(), camera.getFy(), camera.getCx(), camera.getCy(), camera.getS(), &trk_),
        "xk_trk_create");
  const int rc = xk_trk_klt_setup(trk_, (int)camera.getWidth(), (int)camera.getHeight(), win_w, win_h, max_level, max_iter, eps, min_eig_thr);
  if (rc != XK_OK) {
    xk_trk_destroy(trk_);
    check(xk_, rc, "xk_trk_klt_setup");
  }
}

FeatureTracker::~FeatureTracker() { xk_trk_destroy(trk_); }

void FeatureTracker::pushImage(const uint8_t *image, int stride) { check(xk_, xk_trk_push_image(trk_, image, stride), "xk_trk_push_image"); }

std::pair<FeatureList, FeatureList> FeatureTracker::track(const FeatureList &previous, std::vector<int> *kept_indices) {
  const size_t n = previous.size();
  if (n > status_.size()) throw std::runtime_error("FeatureTracker::track: more features than max_features");
  for (size_t i = 0; i < n; ++i) {                            // Feature::getDistPoint2f, tracker.cpp:629-633
    prev_in_[2 * i] = (float)previous[i].getXDist(); prev_in_[2 * i + 1] = (float)previous[i].getYDist();
  }
  int n_kept = 0;
  check(xk_, xk_trk_track(trk_, prev_in_.data(), (int)n, cur_.data(), status_.data(), min_eig_.data(), keep_.data(), kept_prev_.data(),
                          kept_cur_.data(), &n_kept),
        "xk_trk_track");
  std::pair<FeatureList, FeatureList> out;                    // features1 after the erase loop, features2 (:658-686)
  out.first.reserve((size_t)n_kept); out.second.reserve((size_t)n_kept);
  for (int k = 0; k < n_kept; ++k) {
    out.first.push_back(previous[(size_t)keep_[k]]);
    out.second.emplace_back(0.0, 0.0, kept_cur_[2 * k], kept_cur_[2 * k + 1]);
  }
  if (kept_indices) kept_indices->assign(keep_.begin(), keep_.begin() + n_kept);
  return out;
}
