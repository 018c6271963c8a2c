// x/vision/tracker.h -- Tracker::track (src/x/vision/tracker.cpp:134-306) on the mirror: an image goes in, the frame's MatchList comes
// out.  Pyramid level 0.  The whole frame -- pyramid, Lucas-Kanade tracking, removeOverflowFeatures, the re-detection with its
// descriptors, the undistortion and the fundamental-matrix RANSAC -- runs on the GPU behind xk_trk_frame (include/xk.h),
// and previous_features_ (tracker.cpp:299) stays on the device between frames.  After setPhotometric it is the frame of a
// PHOTOMETRIC_CALI build, calibrateImage included, behind xk_trk_photo_frame.  There is no CPU fallback.
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
  // The reference's parameters (tracker.h:75-79, :234-261): outlier_method 4 (cv::LMEDS) is least median of squares, which ignores
  // outlier_param1; every other value is RANSAC (8 is cv::RANSAC; cv::FM_7POINT and FM_8POINT are out of scope: DESIGN 3.10).
  // outlier_param1 is the RANSAC threshold in pixels; outlier_param2, the confidence, has no counterpart: all n_hyp hypotheses are
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
  // PHOTOMETRIC_CALI: calibrateImage on every image after the first (tracker.cpp:186-190).  kernel_size is intensities_kernel_size_
  // (tracker.h:366), epsilon_gap and epsilon_base the drift parameters of IRPhotoCalib, n_hyp_photo the most hypotheses of a frame's
  // gain estimate, fast_detection_delta_photo the FAST threshold once gains were estimated (tracker.cpp:848; < 0: no switch).  From
  // then on track() goes through xk_trk_photo_frame and every TrackedFeature of a match carries its getIntensity().
  void setPhotometric(int kernel_size, double epsilon_gap, double epsilon_base, int n_hyp_photo, int fast_detection_delta_photo = -1);
  // The second Lucas-Kanade parameter set of a PHOTOMETRIC_CALI build (win_size_photo_, max_level_photo_, min_eig_thr_photo_,
  // tracker.cpp:641-651; xk_trk_klt_second).  It is forwarded before the photometric setups; the photometric frames then switch to it
  // on the device from the frame of the first gain estimate on, with no further call.  Without setPhotometric the frames stay on the
  // first set.
  void setSecondKlt(int win_size_w, int win_size_h, int max_level, double min_eig_thr);
  // the set the last frame's feature trackings ran with: 1 iff a second set is declared and the calibration was done by then
  int lastKltSet() const { return second_ && photo_ && calibration_.done ? 1 : 0; }
  // IRPhotoCalib's spatial map, as FeatureTracker::setSpatialCalibration, after setPhotometric: every frame accumulates its rows on the
  // device; after a frame that estimated gains track() reads the status and, once the coverage passes thr, runs the estimate and
  // installs the map (synchronous, on the caller's thread)
  void setSpatialCalibration(int div = 16, double thr = 0.9, int max_rows = 1 << 18);
  bool spatialCalibrated() const { return spatial_done_; }
  const xk_photo_spatial_outcome &spatialOutcome() const { return spatial_outcome_; }
  // the seed of the next frame's gain RANSAC (each frame then takes the next one)
  void setPhotoSeed(unsigned long seed) { seed_photo_ = seed; }
  struct Calibration {
    bool estimated = false, done = false;   // gains were estimated by this frame; by a frame so far
    int kept = 0, support = 0;              // features the raw tracking kept, inliers of the estimate
    double a_rel = 1.0, b_rel = 0.0;        // the estimate against the previous frame
    double frame_ab[4] = {0, 0, 0, 0};      // the pair after the drift adjustments, the frame's origin pair
  };
  // the outcome of the last frame's calibrateImage
  const Calibration &calibration() const { return calibration_; }
  // the next tracked image is a first image
  void reset();

  // One image, height rows of stride bytes -> the frame's matches (none on a first image).  Every TrackedFeature of a match is
  // filled: undistorted and distorted pixels, FAST score, pyramid level 0, tile, descriptor (with a description).
  const MatchList &track(const uint8_t *img, int stride, double timestamp, unsigned int frame_number);
  MatchList getMatches() const { return matches_; }
  // the counts of the last frame, and for each match the position of its feature in the previous frame's match list (or -(k + 1)
  // for the k-th feature the frame's re-detection accepted)
  const xk_trk_frame_out &counts() const { return out_; }
  // the device object behind this tracker: what xk_trk_tracks_manage_frame takes, so that the frame's matches stay on the device
  // (x::ResidentTrackManager::manageFrame); owned by the tracker
  xk_trk *handle() const { return trk_; }
  int maxFeatures() const { return max_features_; }
  const std::vector<int> &origins() const { return origin_v_; }
  int getImgId() const { return img_id_; }
  // the winner's median and scale of the last frame's outlier removal under outlier_method 4 (zeros: no candidate, nothing kept); false
  // under RANSAC and after a first image
  bool lastLmeds(double *median, double *sigma);

 private:
  void apply();               // the setups behind the parameters, made (again) before the next frame

  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  int width_, height_, max_features_;
  int threshold_, nms_, b_, margin_, n_feat_min_, win_w_, win_h_, max_level_, n_hyp_, outlier_method_;
  double threshold_px_, min_eig_thr_;
  unsigned int tiles_h_ = 1, tiles_w_ = 1, max_per_tile_ = 1u << 30;
  bool described_ = false, centroid_ = false, own_pattern_ = false, dirty_ = true;
  double angle_deg_ = -1.0;
  int edge_ = 31;
  signed char pattern_[1024];
  unsigned long seed_ = 0, seed_photo_ = 0;
  bool photo_ = false, spatial_ = false, spatial_done_ = false;
  bool second_ = false, second_pending_ = false;
  int win_w2_ = 31, win_h2_ = 31, max_level2_ = 2;
  double min_eig_thr2_ = 0.003;
  int photo_kernel_ = 30, photo_hyp_ = 0, photo_threshold_ = -1, spatial_div_ = 16, spatial_rows_ = 0;
  double eps_gap_ = 0.0, eps_base_ = 0.0, spatial_thr_ = 0.9;
  Calibration calibration_;
  xk_photo_spatial_outcome spatial_outcome_ = {};
  xk_trk_photo_frame_out pout_{};
  std::vector<double> prev_int_, cur_int_;
  int img_id_ = 0;
  MatchList matches_;
  xk_trk_frame_out out_{};
  std::vector<double> prev_xy_, cur_xy_, prev_dist_, cur_dist_;
  std::vector<int> score_, origin_, tiles_, origin_v_;
  std::vector<unsigned char> desc_;
};
}  // namespace x
