// Mirror of the outlier removal of src/x/vision/tracker.cpp:233-293; the arithmetic runs in libxk.so.
#include "x/vision/match_filter.h"

#include <stdexcept>
#include <string>

using namespace x;

static void check(xk_handle *h, int rc, const char *what) {
  if (rc != XK_OK) throw std::runtime_error(std::string(what) + ": " + xk_strerror(rc) + " (" + (h ? xk_last_error(h) : "") + ")");
}

MatchFilter::MatchFilter(xk_handle *xk, const Camera &camera, int max_matches, double outlier_param1, int n_hyp, unsigned long seed,
                         int outlier_method)
    : xk_(xk), threshold_(outlier_param1), n_hyp_(n_hyp), seed_(seed) {
  check(xk_, xk_trk_create(xk_, max_matches, camera.getFx(), camera.getFy(), camera.getCx(), camera.getCy(), camera.getS(), &trk_),
        "xk_trk_create");
  const size_t m = (size_t)max_matches;                       // (>= 1 here: xk_trk_create refused anything else)
  prev_in_.resize(2 * m); cur_in_.resize(2 * m); prev_out_.resize(2 * m); cur_out_.resize(2 * m);
  mask_.resize(m); keep_.resize(m);
  if (camera.getModel() != XK_CAM_FOV) {                        // the camera's lens (Camera::setDistortion)
    const std::vector<double> k = camera.getCoeffs();
    const int rc = xk_trk_camera_model(trk_, camera.getModel(), k.data(), (int)k.size());
    if (rc != XK_OK) {
      xk_trk_destroy(trk_);
      check(xk_, rc, "xk_trk_camera_model");
    }
  }
  if (outlier_method == XK_TRK_LMEDS) {
    const int rc = xk_trk_outlier_method(trk_, XK_TRK_LMEDS);
    if (rc != XK_OK) {
      xk_trk_destroy(trk_);
      check(xk_, rc, "xk_trk_outlier_method");
    }
  }
}

void MatchFilter::setOutlierMethod(int outlier_method) {
  check(xk_, xk_trk_outlier_method(trk_, outlier_method == XK_TRK_LMEDS ? XK_TRK_LMEDS : XK_TRK_RANSAC), "xk_trk_outlier_method");
}

bool MatchFilter::lastLmeds(double *median, double *sigma) {
  double last[2] = {0.0, 0.0};
  if (xk_trk_fundamental_medians(trk_, 0, 0, nullptr, last) != XK_OK) return false;
  if (median) *median = last[0];
  if (sigma) *sigma = last[1];
  return true;
}

MatchFilter::~MatchFilter() { xk_trk_destroy(trk_); }

MatchList MatchFilter::filter(const FeatureList &previous, const FeatureList &current, std::vector<int> *kept_indices) {
  if (previous.size() != current.size()) throw std::runtime_error("MatchFilter::filter: feature lists of different size");
  const size_t n = previous.size();                            // n_matches, tracker.cpp:243
  if (n > mask_.size()) throw std::runtime_error("MatchFilter::filter: more pairs than max_matches");
  for (size_t i = 0; i < n; ++i) {
    prev_in_[2 * i] = previous[i].getXDist(); prev_in_[2 * i + 1] = previous[i].getYDist();
    cur_in_[2 * i] = current[i].getXDist(); cur_in_[2 * i + 1] = current[i].getYDist();
  }
  int n_inliers = 0;
  check(xk_, xk_trk_filter_matches(trk_, prev_in_.data(), cur_in_.data(), (int)n, threshold_, n_hyp_, seed_, mask_.data(), keep_.data(),
                                   prev_out_.data(), cur_out_.data(), &n_inliers),
        "xk_trk_filter_matches");
  MatchList matches((size_t)n_inliers);                        // :282-293 (the result list is the caller's, as in the reference)
  for (int k = 0; k < n_inliers; ++k) {
    Match &m = matches[(size_t)k];
    m.previous = previous[(size_t)keep_[k]];
    m.current = current[(size_t)keep_[k]];
    m.previous.setX(prev_out_[2 * k]); m.previous.setY(prev_out_[2 * k + 1]);
    m.current.setX(cur_out_[2 * k]); m.current.setY(cur_out_[2 * k + 1]);
  }
  if (kept_indices) kept_indices->assign(keep_.begin(), keep_.begin() + n_inliers);
  return matches;
}
