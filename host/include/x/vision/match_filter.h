// x/vision/match_filter.h -- the outlier removal of x::Tracker::track (src/x/vision/tracker.cpp:233-293) on the mirror:
// undistort the previous and the current feature list (camera.cpp:62-87), cv::findFundamentalMat(pts1, pts2, outlier_method,
// outlier_param1 = 0.3, outlier_param2 = 0.99, mask) on their float casts, keep the masked pairs as the frame's MatchList.
// outlier_method 4 (cv::LMEDS) is least median of squares, which ignores outlier_param1; every other value is RANSAC.
// All of it runs on the GPU behind xk_trk_filter_matches (include/xk.h).  There is no CPU fallback.
#pragma once
#include <vector>

#include "x/vision/camera.h"
#include "xk.h"

namespace x {
class MatchFilter {
 public:
  // outlier_param1: the RANSAC threshold in pixels (tracker.cpp:259-260); n_hyp seven-point hypotheses are all evaluated,
  // which is why the reference's outlier_param2 (prob) has no counterpart
  MatchFilter(xk_handle *xk, const Camera &camera, int max_matches = 1024, double outlier_param1 = 0.3, int n_hyp = 1024,
              unsigned long seed = 0, int outlier_method = XK_TRK_RANSAC);
  ~MatchFilter();
  MatchFilter(const MatchFilter &) = delete;
  MatchFilter &operator=(const MatchFilter &) = delete;

  // previous / current: the tracked pairs, row i of one matched to row i of the other, distorted pixels in getXDist /
  // getYDist.  -> the matches of tracker.cpp:286-293: the kept pairs in input order, getX / getY set to the undistorted
  // pixels.  kept_indices (optional): their positions in the input lists, ascending.
  MatchList filter(const FeatureList &previous, const FeatureList &current, std::vector<int> *kept_indices = nullptr);
  void setSeed(unsigned long seed) { seed_ = seed; }
  // Tracker's outlier_method_ from the next filter() on: 4 is cv::LMEDS, every other value RANSAC
  void setOutlierMethod(int outlier_method);
  // the winner's median and scale of the last filter() if it ran LMedS (zeros: it kept nothing for lack of a candidate); false after RANSAC
  bool lastLmeds(double *median, double *sigma);

 private:
  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  double threshold_;
  int n_hyp_;
  unsigned long seed_;
  // staging for one call, sized once by max_matches: distorted pairs in, kept pairs out
  std::vector<double> prev_in_, cur_in_, prev_out_, cur_out_;
  std::vector<unsigned char> mask_;
  std::vector<int> keep_;
};
}  // namespace x
