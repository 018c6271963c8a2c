// x/vision/tracker.h -- Tracker::track (src/x/vision/tracker.cpp:134-306) on the mirror: an image goes in, the frame's MatchList comes
// out.  A build without PHOTOMETRIC_CALI, pyramid level 0.  The whole frame -- pyramid, Lucas-Kanade tracking, removeOverflowFeatures,
// the re-detection with its descriptors, the undistortion and the fundamental-matrix RANSAC -- runs on the GPU behind xk_trk_frame
// (include/xk.h), and previous_features_ (tracker.cpp:299) stays on the device between frames.  There is no CPU fallback.
// x::FeatureTracker and x::MatchFilter remain the stage-by-stage mirrors.
#pragma once
#include <cstdint>
#include <vector>

#include "x/vision/camera.h"
#include "x/vision/types.h"
#include "xk.h"

namespace x {
class Tracker {
 public:
  // The reference's parameters (tracker.h:75-79, :234-261): outlier_method is cv::RANSAC there and RANSAC here whatever it says;
  // outlier_param1 is the threshold in pixels; outlier_param2, the confidence, has no counterpart: all n_hyp hypotheses are
  // evaluated.  max_features bounds every list of a frame.  term_crit_ is (COUNT + EPS, 30, 0.01) as there.
  Tracker(xk_handle *xk, const Camera &cam, int fast_detection_delta, bool non_max_supp, unsigned int block_half_length,
          unsigned int margin, unsigned int n_feat_min, int outlier_method, double outlier_param1, double outlier_param2,
          int win_size_w, int win_size_h, int max_level, double min_eig_thr, int max_features = 1024, int n_hyp = 1024);
  ~Tracker();
  Tracker(const Tracker &) = delete;
  Tracker &operator=(const Tracker &) = delete;

  // TiledImage::setTileSize and setMaxFeatPerTile of the images the reference's caller hands in (tiled_image.cpp:98-105); the
  // default is one tile that never overflows
  void setTiles(unsigned int n_tiles_h, unsigned int n_tiles_w, unsigned int max_feat_per_tile);
  // PlaceRecognition::compute on every detection (tracker.cpp:440-444), as FeatureTracker::setDescription: the features then carry
  // their descriptors.  The detection's margin is raised to `edge`
  void setDescription(bool centroid_orientation = false, double angle_deg = -1.0, int edge = 31, const signed char *pattern = nullptr);
  // the seed of the next frame's RANSAC (each frame then takes the next one)
  void setSeed(unsigned long seed) { seed_ = seed; }
  // the next tracked image is a first image
  void reset();

  // One image, height rows of stride bytes -> the frame's matches (none on a first image).  Every TrackedFeature of a match is
  // filled: undistorted and distorted pixels, FAST score, pyramid level 0, tile, descriptor (with a description).
  const MatchList &track(const uint8_t *img, int stride, double timestamp, unsigned int frame_number);
  MatchList getMatches() const { return matches_; }
  // the counts of the last frame, and for each match the position of its feature in the previous frame's match list (or -(k + 1)
  // for the k-th feature the frame's re-detection accepted)
  const xk_trk_frame_out &counts() const { return out_; }
  const std::vector<int> &origins() const { return origin_v_; }
  int getImgId() const { return img_id_; }

 private:
  void apply();               // the setups behind the parameters, made (again) before the next frame

  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  int width_, height_, max_features_;
  int threshold_, nms_, b_, margin_, n_feat_min_, win_w_, win_h_, max_level_, n_hyp_;
  double threshold_px_, min_eig_thr_;
  unsigned int tiles_h_ = 1, tiles_w_ = 1, max_per_tile_ = 1u << 30;
  bool described_ = false, centroid_ = false, own_pattern_ = false, dirty_ = true;
  double angle_deg_ = -1.0;
  int edge_ = 31;
  signed char pattern_[1024];
  unsigned long seed_ = 0;
  int img_id_ = 0;
  MatchList matches_;
  xk_trk_frame_out out_{};
  std::vector<double> prev_xy_, cur_xy_, prev_dist_, cur_dist_;
  std::vector<int> score_, origin_, tiles_, origin_v_;
  std::vector<unsigned char> desc_;
};
}  // namespace x
