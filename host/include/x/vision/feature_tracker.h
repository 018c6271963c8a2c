// x/vision/feature_tracker.h -- Tracker::featureTracking (src/x/vision/tracker.cpp:623-690) on the mirror:
// cv::calcOpticalFlowPyrLK(previous image, current image, pts1, pts2, status, err, win_size_, max_level_, term_crit_,
// cv::OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_thr_) on the previous features' distorted pixels, then the pairs that were tracked
// and stayed inside the frame.  All of it runs on the GPU behind xk_trk_push_image / xk_trk_track (include/xk.h); the lists it
// returns are what x::MatchFilter::filter takes.  There is no CPU fallback.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "x/vision/camera.h"
#include "xk.h"

namespace x {
class FeatureTracker {
 public:
  // the image size is the camera's; the other defaults are the reference's (tracker.h:234-261)
  FeatureTracker(xk_handle *xk, const Camera &camera, int max_features = 1024, int win_w = 31, int win_h = 31, int max_level = 2,
                 int max_iter = 30, double eps = 0.01, double min_eig_thr = 0.003);
  ~FeatureTracker();
  FeatureTracker(const FeatureTracker &) = delete;
  FeatureTracker &operator=(const FeatureTracker &) = delete;

  // the next frame, height rows of stride bytes: the current image becomes the previous one (tracker.cpp:302)
  void pushImage(const uint8_t *image, int stride);
  // previous: the features of the previous image, distorted pixels in getXDist / getYDist.  -> the kept features of the
  // previous list and, row for row, where they are in the current image (getXDist / getYDist; getX / getY are left for
  // the undistortion).  kept_indices (optional): their positions in the input list, ascending.
  std::pair<FeatureList, FeatureList> track(const FeatureList &previous, std::vector<int> *kept_indices = nullptr);
  int levels() const { return xk_trk_klt_levels(trk_); }

 private:
  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  // staging for one call, sized once by max_features: points in, everything xk_trk_track reports out
  std::vector<float> prev_in_;
  std::vector<double> cur_, min_eig_, kept_prev_, kept_cur_;
  std::vector<unsigned char> status_;
  std::vector<int> keep_;
};
}  // namespace x
